"""CPU: the shipping library's kernel-argument preload (decagon_amd/_build.py).

The device compile asks for the leading argument dwords of every kernel to be placed in user SGPRs
at wave launch.  How many a kernel got is in its 64-byte kernel descriptor (the `<kernel>.kd`
symbol in the code object's .rodata): the low 7 bits of the 16-bit word at byte 58.  The wave-table
kernels must get their first seven dwords (pairs, desc, ovf, S: what the descriptor and first-pairs
loads need) and the fused decoders their first fourteen (rows, cols, neg_given, alias, n, range,
seed, offset: what the index loads and the draws need).  The flag must not touch the C ABI: the
library still exports every dg_* entry point the header declares.

Descriptor fields and symbol names only: no instruction is looked at here.
"""
import struct
import sys
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

import isa_scan  # noqa: E402

LIB = ROOT / "decagon_amd" / "lib" / "libdecagon_hip.so"
TAB_DWORDS = 7       # pairs, desc, ovf (three pointers) and S
DEC_THROUGH_N = 9    # rows, cols, neg_given, alias (four pointers) and n
DEC_DWORDS = 14      # ... range, seed and offset too: every user SGPR beside the argument pointer's two
DECODERS = ["decoder_hinge_kernelILb1E", "decoder_hinge_kernelILb0E",
            "decoder_rows_hinge_kernelILb1ELi2ELi1E", "decoder_rows_hinge_kernelILb0ELi2ELi1E"]


def _elf_symbols(blob: bytes, table: str):
    """(sections {name: (addr, offset, size)}, symbols {name: (value, size)}) of a little-endian
    ELF64 image; `table` is ".symtab" or ".dynsym"."""
    assert blob[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]

    def text(strtab, at):
        start = heads[strtab][4] + at
        return blob[start:blob.index(b"\0", start)].decode()

    sections = {text(shstrndx, h[0]): (h[3], h[4], h[5]) for h in heads}
    symbols = {}
    for h in heads:
        if text(shstrndx, h[0]) != table:
            continue
        for at in range(h[4], h[4] + h[5], 24):
            name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", blob, at)
            if shndx:  # defined here
                symbols[text(h[6], name)] = (value, size)
    return sections, symbols


@pytest.fixture(scope="module")
def preload_lengths():
    """{kernel symbol: dwords preloaded} over every gfx950 code object of the library."""
    if not LIB.exists():
        pytest.skip("libdecagon_hip.so not built")
    if not (isa_scan.LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm llvm-objdump not available")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in isa_scan.extract_code_objects(LIB, Path(td)):
            blob = co.read_bytes()
            sections, symbols = _elf_symbols(blob, ".symtab")
            addr, offset, size = sections[".rodata"]
            for name, (value, sym_size) in symbols.items():
                if not name.endswith(".kd"):
                    continue
                assert sym_size == 64 and addr <= value and value + 64 <= addr + size, name
                word, = struct.unpack_from("<H", blob, offset + (value - addr) + 58)
                out[name[:-3]] = word & 0x7F
    assert len(out) > 100  # every kernel of the library
    return out


def test_wave_table_kernels_preload_their_first_trip(preload_lengths):
    tab = {k: v for k, v in preload_lengths.items() if "gcn_tab_kernel" in k}
    assert len(tab) >= 8, sorted(tab)  # the POST, DEC, PROJ, PEER and plain instances at both wave counts
    print("gcn_tab_kernel preload lengths:", sorted(set(tab.values())))
    short = {k: v for k, v in tab.items() if v < TAB_DWORDS}
    assert not short, short


def test_fused_decoders_preload_their_first_trip(preload_lengths):
    for needle in DECODERS:
        (name,) = [k for k in preload_lengths if needle in k]
        got = preload_lengths[name]
        print(f"{needle}: {got} dwords preloaded")
        assert got >= DEC_THROUGH_N, (name, got)
        assert got == DEC_DWORDS, (name, got)  # (this toolchain grants all fourteen)


def test_a_kernel_opening_with_a_struct_gets_none(preload_lengths):
    """The reading is not vacuous: the preload stops in front of a by-value struct, so the
    score-only decoder (one DecArgs) keeps its argument read."""
    (name,) = [k for k in preload_lengths if "decoder_score_kernel" in k]
    assert preload_lengths[name] == 0


def test_library_exports_every_declared_entry_point():
    from decagon_amd import abi

    if not LIB.exists():
        pytest.skip("libdecagon_hip.so not built")
    _, exported = _elf_symbols(LIB.read_bytes(), ".dynsym")
    missing = [fn for fn in abi.PROTOTYPES if fn not in exported]
    assert len(abi.PROTOTYPES) >= 78 and not missing, missing
