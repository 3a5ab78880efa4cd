"""CPU: the binding is read from include/decagon_hip.h (decagon_amd/abi.py).  The C++ compiler's
view of the header — struct layouts and every prototype's parameter types — is compared with the
parser's; the parser refuses what it does not know; arguments pack by parameter name."""
import ctypes
import subprocess
from pathlib import Path

import pytest

from test_cpu_host import _declared_symbols

ROOT = Path(__file__).resolve().parents[1]

PROBE = """
#include "decagon_hip.h"
#include <cstddef>
#include <cstdio>
#include <type_traits>
template <class T> void type() {  // size, class (p / i / f) and signedness (s / u; - for no integer)
    if constexpr (std::is_void<T>::value) std::printf(" void");
    else std::printf(" %zu%c%c", sizeof(T),
                     std::is_pointer<T>::value ? 'p' : std::is_integral<T>::value ? 'i'
                     : std::is_floating_point<T>::value ? 'f' : '?',
                     !std::is_integral<T>::value ? '-' : std::is_signed<T>::value ? 's' : 'u');
}
template <class R, class... A> void proto(const char* name, R (*)(A...)) {
    std::printf("P %s", name); type<R>(); (type<A>(), ...); std::printf("\\n");
}
int main() {
@BODY@
    return 0;
}
"""


def _describe(ct) -> str:
    """A ctypes type as the probe prints a C type."""
    if ct is None:
        return "void"
    if ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer):
        kind = "p-"
    elif ct._type_ in "fd":
        kind = "f-"
    else:
        assert ct._type_ in "bBhHiIlLqQ", ct
        kind = "i" + ("s" if ct._type_.islower() else "u")
    return f"{ctypes.sizeof(ct)}{kind}"


@pytest.fixture(scope="module")
def compiler_view(tmp_path_factory):
    """What a host-only C++ compile of the header says: {"S dg_x": [sizeof], "F dg_x field": [offset],
    "P dg_fn": [return type, parameter types ...]}.  No --offload-arch, nothing linked from the library:
    the prototypes are inspected through decltype."""
    from decagon_amd import _build, abi

    try:
        cxx = _build.hipcc()
    except RuntimeError as e:
        pytest.skip(f"no host compiler: {e}")
    lines = []
    for cname, cls in abi.ABI.structs.items():
        lines.append(f'    std::printf("S {cname} %zu\\n", sizeof({cname}));')
        lines += [f'    std::printf("F {cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'    proto("{fn}", static_cast<decltype({fn})*>(nullptr));' for fn in abi.PROTOTYPES]
    tmp = tmp_path_factory.mktemp("abi_probe")
    (tmp / "probe.cpp").write_text(PROBE.replace("@BODY@", "\n".join(lines)))
    subprocess.run([cxx, "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(tmp / "probe.cpp"), "-o",
                    str(tmp / "probe")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp / "probe")], check=True, capture_output=True, text=True).stdout
    view = {}
    for line in out.splitlines():
        words = line.split()
        n_key = {"S": 2, "F": 3, "P": 2}[words[0]]
        view[" ".join(words[:n_key])] = words[n_key:]
    return view


def test_struct_layouts_are_the_compilers(compiler_view):
    from decagon_amd import abi

    assert len(abi.ABI.structs) == 15
    for cname, cls in abi.ABI.structs.items():
        assert compiler_view[f"S {cname}"] == [str(ctypes.sizeof(cls))], cname
        for f, _ in cls._fields_:
            assert compiler_view[f"F {cname} {f}"] == [str(getattr(cls, f).offset)], (cname, f)
    n_fields = sum(len(c._fields_) for c in abi.ABI.structs.values())
    assert sum(k.startswith("F ") for k in compiler_view) == n_fields > 100


def test_prototypes_are_the_compilers(compiler_view):
    """All 78 entry points: the return type's and every parameter's size, class and signedness."""
    from decagon_amd import abi

    assert len(abi.PROTOTYPES) == 78 == sum(k.startswith("P ") for k in compiler_view)
    for fn, p in abi.PROTOTYPES.items():
        assert compiler_view[f"P {fn}"] == [_describe(p.restype)] + [_describe(a) for a in p.argtypes], fn
        assert len(p.names) == len(p.argtypes) == len(set(p.names)), fn


def test_every_parsed_prototype_binds():
    from decagon_amd import _lib, abi

    lib = _lib.load()
    for fn, p in abi.PROTOTYPES.items():
        bound = getattr(lib, fn)
        assert bound.restype is p.restype and list(bound.argtypes) == p.argtypes, fn
        assert _lib.SIGNATURES[fn] == (p.restype, p.argtypes)
    assert sorted(abi.PROTOTYPES) == _declared_symbols()


def test_re_exports_are_the_header_values():
    from decagon_amd import _lib, abi, wavetable

    for name, value in abi.CONSTANTS.items():
        assert getattr(_lib, name) == value, name
    assert _lib.DG_PEER_STATE_WORDS == 64 + 8 * 8 * 16 and _lib.DG_HINGE_WS_BYTES == 16 + 4 * 256
    assert abi.CONSTANTS["DG_CROSS_MAX_OUT"] == 1 << 38 and abi.CONSTANTS["DG_EINVAL"] == -1
    assert "DECAGON_HIP_H" not in abi.CONSTANTS
    for cls in abi.ABI.structs.values():
        assert getattr(_lib, cls.__name__) is cls
    assert _lib.DgEpiTarget.groups.offset == 0 and dict(_lib.DgEpiTarget._fields_)["groups"]._type_ is _lib.DgEpiGroup
    assert dict(_lib.DgWaveTable._fields_)["desc"] is ctypes.c_void_p  # a device array: an address
    assert dict(_lib.DgPeerXchg._fields_)["flags"]._length_ == _lib.DG_PEER_MAX
    assert wavetable.DG_TAB_ROLE_PROJ_BIT == abi.CONSTANTS["DG_TAB_ROLE_PROJ_BIT"] == 30


@pytest.mark.parametrize("bad,needle,line", [
    ("int dg_f(int32_t n,\n         size_t bytes);", "size_t", 5),                      # an unknown parameter type
    ("int dg_f(int32_t n,\n         int (*cb)(int));", "dg_f", 4),                      # a function pointer
    ("typedef struct dg_s {\n    int32_t a;\n    int32_t b : 3;\n} dg_s;", "b : 3", 6),  # a bit field
    ("typedef struct dg_s {\n    struct { int32_t a; } in;\n} dg_s;", "dg_s", 4),       # a nested struct
    ("#define DG_A 1\n#define DG_B (DG_A + DG_C)", "DG_C", 5),                          # an undefined macro
    ("#define DG_A sizeof(int)", "sizeof", 4),
    ("#pragma once", "pragma", 4),
    ("int dg_f(const dg_unknown* p /* HOST */);", "dg_unknown", 4),
    ("int dg_f(int32_t n)\n#define DG_A 1", "dg_f", 4),                                 # no `;`
])
def test_the_parser_refuses_what_it_does_not_know(bad, needle, line):
    """It raises and names the header line (the text starts at line 4); nothing is guessed."""
    from decagon_amd import abi

    text = "#define DG_OK 0\n/* two\n   lines */\n" + bad + "\nint dg_g(void);\n"
    with pytest.raises(abi.AbiError) as e:
        abi.parse(text, "t.h")
    assert str(e.value).startswith(f"t.h:{line}: ") and needle in str(e.value), str(e.value)


def test_the_parser_reads_the_documented_subset():
    from decagon_amd import abi

    got = abi.parse("""
#define DG_N (1ll << 3)   /* a comment, with a comma */
#define DG_M (2 * DG_N - 1u + 0x10)
typedef struct dg_in { float* p; int64_t a, b; } dg_in;
typedef struct dg_out {
    const dg_in* host;      /* HOST array */
    const dg_in* dev;       /* device */
    uint32_t* words[DG_N];
    int32_t tail[2];
} dg_out;
struct dg_out;
int64_t dg_f(const struct dg_out* o /* HOST, may be NULL */, const dg_in* d, void** out /* HOST out */,
             int32_t* /* HOST out */ n, const int32_t* idx, unsigned long long seed, double x, void* stream);
uint32_t dg_g(void);
""")
    assert got.constants == {"DG_N": 8, "DG_M": 31}
    d_in, d_out = got.structs["dg_in"], got.structs["dg_out"]
    assert (d_in.__name__, d_out.__name__) == ("DgIn", "DgOut")
    assert d_in._fields_ == [("p", ctypes.c_void_p), ("a", ctypes.c_int64), ("b", ctypes.c_int64)]
    assert d_out._fields_ == [("host", ctypes.POINTER(d_in)), ("dev", ctypes.c_void_p),
                              ("words", ctypes.c_void_p * 8), ("tail", ctypes.c_int32 * 2)]
    f = got.prototypes["dg_f"]
    assert f.restype is ctypes.c_int64 and f.names == ("o", "d", "out", "n", "idx", "seed", "x", "stream")
    assert f.argtypes == [ctypes.POINTER(d_out), ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                          ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double,
                          ctypes.c_void_p]
    assert got.prototypes["dg_g"] == (ctypes.c_uint32, [], ())


def test_pack_builds_arguments_by_name():
    from decagon_amd import _lib, abi

    # the positions kernels.PreparedDecoderHinge used to patch by number
    assert _lib.arg_index("dg_decoder_hinge_f32", "seed") == 9
    assert _lib.arg_index("dg_decoder_hinge_f32", "offset") == 10
    assert _lib.arg_index("dg_decoder_hinge_rows_f32", "seed") == 9
    assert _lib.arg_index("dg_decoder_grad_seg_xent_f32", "coef") == 24
    with pytest.raises(TypeError, match="no parameter 'coef'"):
        _lib.arg_index("dg_decoder_grad_seg_f32", "coef")
    names = abi.PROTOTYPES["dg_hinge_loss_f32"].names
    assert names == ("pos", "neg", "n", "margin", "loss", "stream")
    values = dict(stream=None, loss=5, margin=0.5, n=3, neg=2, pos=1)
    assert _lib.pack("dg_hinge_loss_f32", **values) == [1, 2, 3, 0.5, 5, None]
    with pytest.raises(TypeError, match=r"missing arguments \['margin'\]"):
        _lib.pack("dg_hinge_loss_f32", **{k: v for k, v in values.items() if k != "margin"})
    with pytest.raises(TypeError, match=r"unknown arguments \['neg_weight'\]"):
        _lib.pack("dg_hinge_loss_f32", neg_weight=1.0, **values)


def test_desc_dtype_is_dg_tab_desc():
    from decagon_amd import abi, wavetable

    cls = abi.ABI.structs["dg_tab_desc"]
    assert ctypes.sizeof(cls) == wavetable.DESC.itemsize == 64
    assert [f for f, _ in cls._fields_] == list(wavetable.DESC.names)
    for f, ct in cls._fields_:
        dt, offset = wavetable.DESC.fields[f][:2]
        assert offset == getattr(cls, f).offset and dt.itemsize == ctypes.sizeof(ct), f
