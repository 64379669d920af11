"""The multivector entry points (include/mi355_multivec.h, the companion header of mi355_ann.h) checked the way
tests/test_abi.py and tests/test_rust_binding.py check mi355_ann.h: the library exports every declared entry point
under its C name, each definition is a function-try-block closed by the exception barrier, mi355_ann.h (the v6
surface) declares none of them, and integration/mi355_multivec_sys.rs is what the generator produces and agrees with a
C program compiled against the header on struct layout, function set and argument counts.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

from lancedb_amd import _abi, _lib
from tests.test_rust_binding import _repr_c_layout, _rs_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
ANN_HEADER = os.path.join(ROOT, "include", "mi355_ann.h")
MV_HEADER = os.path.join(ROOT, "include", "mi355_multivec.h")
MV_RS = os.path.join(ROOT, "integration", "mi355_multivec_sys.rs")
UNIT = os.path.join(ROOT, "lancedb_amd", "csrc", "ann_multivec.hip")


def _header_protos(path):
    hdr = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for n, a in re.findall(r"\bu?int32_t\s+(mi355_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.S):
        a = " ".join(a.split())
        out[n] = 0 if a == "void" else len(a.split(","))
    return out


def test_header_declares_the_export_list_and_mi355_ann_h_none_of_it():
    assert set(_header_protos(MV_HEADER)) == set(_abi.MULTIVEC_SYMBOLS)
    assert not set(_abi.MULTIVEC_SYMBOLS) & set(_abi.EXPORTED_SYMBOLS)
    assert "mi355_multivec" not in open(ANN_HEADER).read()


def test_library_exports_the_c_names():
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in _abi.MULTIVEC_SYMBOLS:
        assert getattr(L, name) is not None
    r = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if r.returncode == 0:
        exported = set(re.findall(r"\bT (mi355_multivec_\w+)$", r.stdout, flags=re.M))
        assert exported == set(_abi.MULTIVEC_SYMBOLS)


def test_every_entry_point_has_the_exception_barrier():
    """Each definition is a function-try-block closed by MI355_MV_ABI_GUARD naming itself, and that macro is
    MI355_ABI_GUARD with the full entry-point name."""
    src = open(UNIT).read()
    assert re.search(r'#define MI355_MV_ABI_GUARD\(suffix\) MI355_ABI_GUARD\("mi355_multivec_" suffix\)', src)
    assert '#include "../../include/mi355_multivec.h"' in src  # (the C linkage comes from its extern "C" block)
    defs = re.findall(r"^int32_t (mi355_multivec_\w+)\(", src, flags=re.M)
    guards = ["mi355_multivec_" + g for g in re.findall(r'MI355_MV_ABI_GUARD\("(\w+)"\)', src)]
    assert sorted(defs) == sorted(guards) == sorted(_abi.MULTIVEC_SYMBOLS)
    for d in defs:
        assert re.search(r"^int32_t " + d + r"\([^{;]*\) try \{", src, flags=re.M), d
    # no other unit defines them
    csrc = os.path.dirname(UNIT)
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")) and f != os.path.basename(UNIT):
            assert not re.search(r"\bmi355_multivec_\w+\([^;]*\)\s*(?:try\s*)?\{", open(os.path.join(csrc, f)).read()), f


def test_committed_rust_module_is_what_the_generator_produces():
    import gen_rust_sys
    assert open(MV_RS).read() == gen_rust_sys.generate_multivec(), "stale: run python scripts/gen_rust_sys.py"


def test_rust_struct_layout_matches_a_c_probe_of_the_header(tmp_path):
    structs = _rs_structs(open(MV_RS).read())
    assert set(structs) == {"mi355_multivec_desc"}
    lines = ['#include "mi355_multivec.h"', "#include <stddef.h>", "#include <stdio.h>", "int main(void) {"]
    for s, fields in structs.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        for f, _, _ in fields:
            lines.append(f'  printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));')
    lines += ["  return 0;", "}"]
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.dirname(MV_HEADER), str(c), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = tuple(int(x) for x in v)
    hdr = re.sub(r"/\*.*?\*/", " ", open(MV_HEADER).read(), flags=re.S)
    for s, fields in structs.items():
        layout, size = _repr_c_layout(fields)
        assert got[s] == (size,) and size == C.sizeof(_abi.MultivecDesc)
        for f, off, sz in layout:
            assert got[f"{s}.{f}"] == (off, sz), (s, f)
            assert getattr(_abi.MultivecDesc, f).offset == off, f
        body = re.search(r"typedef\s+struct\s+" + s + r"\s*\{(.*?)\}\s*" + s + r"\s*;", hdr, flags=re.S).group(1)
        assert sum(len(d.split(",")) for d in body.split(";") if d.strip()) == len(fields)


def test_rust_function_set_and_argument_counts_match_the_header():
    text = open(MV_RS).read()
    rs = {n: (0 if not a.strip() else len(a.split(","))) for n, a in re.findall(r"pub fn (mi355_\w+)\(([^)]*)\) -> \w+;", text)}
    assert rs == _header_protos(MV_HEADER) and set(rs) == set(_abi.MULTIVEC_SYMBOLS)
    assert "pub fn mi355_multivec_search(mv: *mut mi355_multivec, queries: *const f32, n_queries: u32, n_qvec: u32, " \
           "params: *const mi355_search_params, out_rowids: *mut u64, out_dist: *mut f32, out_counts: *mut u32) -> i32;" in text
    assert "use super::mi355_sys::{mi355_search_params};" in text
