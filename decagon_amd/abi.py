"""The C ABI as include/decagon_hip.h declares it, parsed once at import: constants, structs and
prototypes.  Host only and standard library only; nothing here loads the shared library.

include/decagon_hip_ext.h, the entry points added after the 78 of ABI 39, is parsed by the same
parser into a table of its own (EXT), with the first header's constants and structs in scope; each
later extension header (EXT_HEADERS, in order: decagon_hip_ext2.h is EXT2) likewise, with every
earlier table in scope.

The parser accepts the subset of C the header is written in and raises AbiError
with the header line on anything else: it never guesses a type.
"""
from __future__ import annotations

import ctypes
import re
from ctypes import POINTER, c_void_p
from typing import Dict, List, NamedTuple, Optional, Tuple

from . import _build

HEADER = _build.INCLUDE / "decagon_hip.h"
EXT_HEADER = _build.INCLUDE / "decagon_hip_ext.h"
EXT_HEADERS = (EXT_HEADER, _build.INCLUDE / "decagon_hip_ext2.h")  # in the order they include one another

_INTS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
         "uint64_t": ctypes.c_uint64, "unsigned long long": ctypes.c_uint64, "uint16_t": ctypes.c_uint16}
_SCALARS = {**_INTS, "float": ctypes.c_float, "double": ctypes.c_double}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
# one top-level item: a directive | a free HOST comment or an extern "C" brace | a declaration up to its `;`
_ITEM = re.compile(r'(?:(#[^\n]*)|(@HOST|\}|extern\s*"C"\s*\{)|([^;#{}]*(?:\{[^{}]*\}[^;#{}]*)?;))')
_SPACE = re.compile(r"\s*")
_DEFINE = re.compile(r"#\s*define\s+(\w+)\s*(.*)")
_IGNORED = re.compile(r"#\s*(include|ifdef|ifndef|endif)\b")
_GUARD = re.compile(r"DECAGON_HIP(_[A-Z0-9]+)*_H$")  # DECAGON_HIP_H, DECAGON_HIP_EXT_H
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)\s*;$", re.S)
_FIELD = re.compile(r"([^;]*);[ \t]*(@HOST)?")
_PROTO = re.compile(r"([^()]*)\(([^()]*)\)\s*;$")
_TOKEN = re.compile(r"@HOST|[A-Za-z_]\w*|\d\w*|<<|[^\s\w]")
_NAME = re.compile(r"[A-Za-z_]\w*$")
_NUMBER = re.compile(r"(0[xX][0-9a-fA-F]+|\d+)[uUlL]*$")
_PREC = {"<<": 1, "+": 2, "-": 2, "*": 3}


class AbiError(ValueError):
    pass


class Prototype(NamedTuple):
    restype: Optional[type]
    argtypes: List[type]
    names: Tuple[str, ...]


class Abi(NamedTuple):
    constants: Dict[str, int]         # DG_NAME -> value
    structs: Dict[str, type]          # dg_name -> its ctypes.Structure (class DgName)
    prototypes: Dict[str, Prototype]  # dg_name -> types and parameter names


def _evaluate(toks: List[str], consts: Dict[str, int], at: str) -> int:
    """An integer expression over literals, earlier macros, parentheses and + - * <<."""
    toks = toks + [""]

    def atom() -> int:
        t = toks.pop(0)
        if t == "(":
            v = expr(0)
            if toks.pop(0) != ")":
                raise AbiError(f"{at}: unbalanced parenthesis")
            return v
        if t == "-":
            return -atom()
        if _NUMBER.match(t):
            return int(_NUMBER.match(t).group(1), 0)
        if t not in consts:
            raise AbiError(f"{at}: `{t}` is neither an integer literal nor an earlier macro")
        return consts[t]

    def expr(floor: int) -> int:
        v = atom()
        while _PREC.get(toks[0], -1) >= floor:
            op = toks.pop(0)
            r = expr(_PREC[op] + 1)
            v = v << r if op == "<<" else v + r if op == "+" else v - r if op == "-" else v * r
        return v

    v = expr(0)
    if toks != [""]:
        raise AbiError(f"{at}: unexpected `{toks[0]}` in an integer expression")
    return v


def _declarator(text: str, consts, at: str):
    """`const T* name[N]` -> (T, pointer depth, name, N or None)."""
    toks = [t for t in _TOKEN.findall(text) if t not in ("const", "struct", "@HOST")]
    dim = None
    if "[" in toks and toks[-1] == "]":
        k = toks.index("[")
        dim, toks = _evaluate(toks[k + 1:-1], consts, at), toks[:k]
    words = [t for t in toks[:-1] if t != "*"]
    stars = len(toks) - 1 - len(words)
    if not words or not all(_NAME.match(t) for t in words + toks[-1:]) or toks[:-1] != words + ["*"] * stars:
        raise AbiError(f"{at}: cannot read the declaration `{' '.join(text.split())}`")
    return " ".join(words), stars, toks[-1], dim


def _ctype(base: str, stars: int, host: bool, param: bool, structs, at: str):
    """A pointer is a device address (c_void_p, passed as an int) unless its comment says HOST and
    it points to a dg_ struct or, as a parameter, to an integer; void** is a host out-parameter."""
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 2 and base == "void" and param:
        return POINTER(c_void_p)
    if stars == 1 and base in structs:
        return POINTER(structs[base]) if host else c_void_p
    if stars == 1 and (base in _SCALARS or base == "void"):
        return POINTER(_INTS[base]) if host and param and base in _INTS else c_void_p
    raise AbiError(f"{at}: unknown type `{base}{'*' * stars}`")


def _struct(name: str, body: str, abi: Abi, where, line: int) -> None:
    fields, end = [], 0
    for m in _FIELD.finditer(body):  # the HOST marker of a field is the comment after its `;`
        at, end = where(line + body.count("\n", 0, m.end(1))), m.end()
        first, *more = m.group(1).split(",")
        base, stars, fname, dim = _declarator(first, abi.constants, at)
        members = [(stars, fname, dim)] + [_declarator(f"{base} {d}", abi.constants, at)[1:] for d in more]
        for stars, fname, dim in members:  # (`int32_t rank, world;`)
            ct = _ctype(base, stars, bool(m.group(2)), False, abi.structs, at)
            fields.append((fname, ct if dim is None else ct * dim))
    if body[end:].replace("@HOST", "").strip():
        raise AbiError(f"{where(line + body.count(chr(10), 0, end))}: a field of {name} without `;`")
    cls = "".join(p.capitalize() for p in name.split("_"))
    abi.structs[name] = type(cls, (ctypes.Structure,), {"_fields_": fields})


def _prototype(head: str, params: str, abi: Abi, where, line: int) -> None:
    base, stars, name, _ = _declarator(head, abi.constants, where(line))
    restype = None if (base, stars) == ("void", 0) else _ctype(base, stars, False, False, abi.structs, where(line))
    argtypes, names, line = [], [], line + head.count("\n")
    for p in [] if params.strip() == "void" else params.split(","):
        at = where(line + p.count("\n", 0, len(p) - len(p.lstrip())))
        base, stars, pname, dim = _declarator(p, abi.constants, at)
        if dim is not None:
            raise AbiError(f"{at}: array parameter `{pname}`")
        argtypes.append(_ctype(base, stars, "@HOST" in p, True, abi.structs, at))
        names.append(pname)
        line += p.count("\n")
    abi.prototypes[name] = Prototype(restype, argtypes, tuple(names))


def parse(text: str, name: str = HEADER.name, base: Optional[Abi] = None) -> Abi:
    """Constants, structs and prototypes of header `text`; `name` prefixes the error messages.
    With `base`, the table of a header that `text` includes, that header's constants and structs
    are in scope; the result holds only what `text` itself declares."""
    def comment(m):  # keep a HOST marker and the line count, drop the words
        return ("@HOST" if re.search(r"\bHOST\b", m.group()) else " ") + "\n" * m.group().count("\n")

    text = _COMMENT.sub(comment, text).rstrip()
    where = lambda line: f"{name}:{line}"  # noqa: E731
    abi, protos, pos = Abi(dict(base.constants) if base else {}, dict(base.structs) if base else {}, {}), [], 0
    while pos < len(text):
        pos = _SPACE.match(text, pos).end()
        m, line = _ITEM.match(text, pos), text.count("\n", 0, pos) + 1
        if m is None:
            raise AbiError(f"{where(line)}: cannot classify `{text[pos:].splitlines()[0][:80]}`")
        pos, (directive, _, decl) = m.end(), m.groups()
        if directive:
            d = _DEFINE.match(directive)
            if d and d.group(1).startswith("DG_"):
                abi.constants[d.group(1)] = _evaluate(_TOKEN.findall(d.group(2)), abi.constants, where(line))
            elif not (d and _GUARD.match(d.group(1)) and not d.group(2).strip()) and not _IGNORED.match(directive):
                raise AbiError(f"{where(line)}: unsupported directive `{directive}`")
        elif decl:
            s, p = _STRUCT.match(decl), _PROTO.match(decl)
            if s and s.group(1) == s.group(3):
                _struct(s.group(1), s.group(2), abi, where, line + decl.count("\n", 0, s.start(2)))
            elif p and not decl.startswith("typedef"):
                protos.append((p.group(1), p.group(2), line))  # typed once every struct is known
            elif not re.match(r"struct\s+\w+\s*;$", decl):  # (a forward declaration says nothing)
                raise AbiError(f"{where(line)}: cannot classify `{' '.join(decl.split())[:80]}`")
    for head, params, line in protos:
        _prototype(head, params, abi, where, line)
    if base:
        own = lambda table, seen: {k: v for k, v in table.items() if k not in seen}  # noqa: E731
        return Abi(own(abi.constants, base.constants), own(abi.structs, base.structs), abi.prototypes)
    return abi


ABI = parse(HEADER.read_text())
CONSTANTS, PROTOTYPES = ABI.constants, ABI.prototypes
STRUCTS = {cls.__name__: cls for cls in ABI.structs.values()}  # by class name: DgRelGroup, ...
SIGNATURES = {name: (p.restype, p.argtypes) for name, p in PROTOTYPES.items()}


def _parse_extensions(headers) -> List[Abi]:
    """One table per extension header, in order; each is parsed with every earlier table in scope
    and may redeclare none of their prototypes."""
    scope, tables = ABI, []
    for path in headers:
        ext = parse(path.read_text(), path.name, base=scope)
        again = set(ext.prototypes) & set(scope.prototypes)
        if again:
            raise AbiError(f"{path.name} redeclares {sorted(again)}")
        tables.append(ext)
        scope = Abi({**scope.constants, **ext.constants}, {**scope.structs, **ext.structs},
                    {**scope.prototypes, **ext.prototypes})
    return tables


EXTENSIONS = _parse_extensions(EXT_HEADERS)
EXT, EXT2 = EXTENSIONS  # added after the 78 of ABI 39: the filtered edge rank; a node's best partners
ALL_PROTOTYPES = {**PROTOTYPES}  # every table: what _lib types, packs and indexes
globals().update(CONSTANTS)
globals().update(STRUCTS)
for _ext in EXTENSIONS:
    ALL_PROTOTYPES.update(_ext.prototypes)
    globals().update(_ext.constants)
    globals().update({cls.__name__: cls for cls in _ext.structs.values()})
