"""The GEMM launch contract, checked where there is no GPU: the pinned acceptance table of
tests/gemm_conformance_cases.py equals what lgd_gemm_check answers, the tile codes are exactly ops.TILE_NAMES, and the
"exact" data of every form really is exact — which is what entitles tests/test_gemm_conformance_gpu.py to compare
with zero tolerance."""
import os
import sys

import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_conformance_cases as gcc  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _library():
    """The acceptance matrix is the library's answer (lgd_gemm_check): host code, no GPU."""
    import __graft_entry__ as ge
    ge.build()


def test_pinned_acceptance_table_is_what_the_library_answers():
    pinned = gcc.pinned()
    assert list(pinned) == list(gcc.FORMS), "the pinned table has one row per form, in order"
    diff = []
    for name, form in gcc.FORMS.items():
        assert sorted(pinned[name]) == gcc.TILES, name
        for tile, cell in zip(gcc.TILES, gcc.acceptance_row(form)):
            if pinned[name][tile] != cell:
                diff.append((name, tile, pinned[name][tile], cell))
    assert not diff, f"(form, code, pinned, library): {diff}"


def test_tile_codes_are_exactly_tile_names():
    """The codes the library accepts on a plain contiguous descriptor, among 1..79, are the ones ops.TILE_NAMES names."""
    p = gcc.P
    accepted = [t for t in range(1, 80) if ops.gemm_accepts(ops.gemm_desc(p, p, p, 512, 640, 640, splits=1, tile=t))]
    assert accepted == sorted(ops.TILE_NAMES)
    assert ops.gemm_accepts(ops.gemm_desc(p, p, p, 512, 640, 640, splits=1, tile=0))          # 0 = the library's heuristic


# the profiler's kernel names (profiles/, tools/ and bench.py's roofline key on them), pinned: code, then the name
PINNED_TILE_NAMES = """
1 gemm_kernel<4,4> 128x128
2 gemm_kernel<4,2> 128x64
3 gemm_kernel<2,4> 64x128
4 gemm_kernel<2,2> 64x64
5 gemm_kernel<1,4> 32x128
6 gemm_kernel<4,5> 128x160
7 gemm_kernel<2,5> 64x160
17 gemm_dma_kernel<4,4,2> 128x128
18 gemm_dma_kernel<4,2,2> 128x64
19 gemm_dma_kernel<2,4,2> 64x128
20 gemm_dma_kernel<2,2,2> 64x64
21 gemm_dma_kernel<1,4,2> 32x128
22 gemm_dma_kernel<4,5,2> 128x160
23 gemm_dma_kernel<2,5,2> 64x160
25 gemm_dma_kernel<4,10,4> 256x320
26 gemm_dma_kernel<4,4,4> 256x128
33 gemm_pipe_kernel<4,5,4,2,3> 256x160
34 gemm_pipe_kernel<4,4,4,2,3> 256x128
35 gemm_pipe_kernel<4,2,4,2,4> 256x64
37 gemm_pipe_kernel<2,5,4,2,4> 128x160
38 gemm_pipe_kernel<2,4,4,2,4> 128x128
39 gemm_pipe_kernel<2,2,4,2,5> 128x64
40 gemm_pipe_kernel<1,5,4,2,5> 64x160
41 gemm_pipe_kernel<1,4,4,2,5> 64x128
42 gemm_pipe_kernel<1,2,4,2,6> 64x64
44 gemm_pipe_kernel<4,8,4,2,2> 256x256
45 gemm_pipe_kernel<2,4,4,2,2> 128x128 x2/CU
46 gemm_phase_kernel<8,4> 256x256
47 gemm_phase_kernel<8,5> 256x320
"""


def test_the_tile_table_carries_the_pinned_names():
    """lgd_gemm_tile enumerated to its end: unique codes, the block shape its name states, LGD_ERR_ARG past the end, and
    the 29 (code, name) pairs byte for byte; ops.TILE_NAMES is that table in code order."""
    import ctypes as C
    from lgd_amd import _lib
    lib = _lib.load()
    code, bm, bn, name, rows = C.c_int(), C.c_int(), C.c_int(), C.create_string_buffer(128), []
    while lib.lgd_gemm_tile(len(rows), C.byref(code), C.byref(bm), C.byref(bn), name, len(name)) == 0:
        assert len(name.value) < len(name) - 1
        rows.append((code.value, bm.value, bn.value, name.value.decode()))
    for bad in (-1, len(rows), len(rows) + 5):
        assert lib.lgd_gemm_tile(bad, C.byref(code), C.byref(bm), C.byref(bn), name, len(name)) == -1, bad
    assert lib.lgd_gemm_tile(0, None, None, None, None, 0) == 0                   # every output is optional
    short = C.create_string_buffer(b"#" * 8, 8)
    assert lib.lgd_gemm_tile(0, None, None, None, short, 5) == 0
    assert short.raw[:5] == rows[0][3].encode()[:4] + b"\0" and short.raw[5:] == b"###"
    pinned = [ln.split(" ", 1) for ln in PINNED_TILE_NAMES.strip().splitlines()]
    assert len(pinned) == 29 and sorted((c, nm) for c, _, _, nm in rows) == [(int(c), nm) for c, nm in pinned]
    assert list(ops.TILE_NAMES.items()) == [(int(c), nm) for c, nm in pinned]
    for c, m, n, nm in rows:
        assert nm.split(" ")[1] == f"{m}x{n}", (c, nm)


def test_acceptance_floors():
    """No code and no form may drop out of the matrix unnoticed: the minima of the pinned table."""
    pinned = gcc.pinned()
    per_code = {t: sum(pinned[n][t] != "." for n in pinned) for t in gcc.TILES}
    per_form = {n: sum(c != "." for c in pinned[n].values()) for n in pinned}
    assert min(per_code.values()) == gcc.MIN_FORMS_PER_CODE, per_code
    assert min(per_form.values()) == gcc.MIN_CODES_PER_FORM, per_form
    assert gcc.MIN_FORMS_PER_CODE >= 9 and gcc.MIN_CODES_PER_FORM >= 14
    # every form of the issue's list is there, with the pair modes on five of them
    for name in ("plain_k64", "plain_k192", "plain_k448", "plain_k72", "plain_n4", "tiny_m", "strided", "inplace", "res_f32",
                 "out_f32_bias2", "geglu", "geglu_res", "rownorm", "rownorm_geglu", "two_src", "two_src_small", "conv_same",
                 "conv_s2", "conv_ups1", "conv_ups2", "conv_two_src", "conv_c8", "conv_split", "batched", "batched_split",
                 "split2", "split4of5", "split_geglu", "split_out_f32"):
        assert name in pinned
    for base in ("plain_k192", "strided", "conv_same", "geglu", "rownorm"):
        assert "half:" + base in pinned and "dup:" + base in pinned


@pytest.mark.parametrize("name", [n for n, f in gcc.FORMS.items() if f.exact])
def test_exact_forms_are_exact(name):
    """Integer / half-integer data: the fp64 reference IS a value of the output type, and the sum of the magnitudes
    of every term of an element stays below 2^24 (with multiples of 0.5: below 2^23 in units of the spacing), so every
    partial sum in any order is an exact fp32 number.  A correct kernel therefore returns the reference bit for bit."""
    c = gcc.FORMS[name].case("exact")
    assert torch.equal(c.rounded_ref(), c.ref)
    assert torch.equal(c.ref * 2, (c.ref * 2).round())                       # multiples of 0.5
    assert 2 * c.s_max < 2 ** 24
    assert float(c.ref.abs().max()) <= 1024                                  # half-integers are exact in fp16 up to 1024


def test_geglu_forms_have_no_exact_mode():
    assert [n for n, f in gcc.FORMS.items() if not f.exact] == [n for n in gcc.FORMS if "geglu" in n]


def test_split4of5_drops_its_empty_trailing_split():
    """Five K tiles over four splits are two tiles each: three splits carry work.  The descriptor keeps what the caller
    asked for; the library normalises its own copy (the workspace is sized for four)."""
    f = gcc.FORMS["split4of5"]
    assert f.K // 64 == 5 and f.splits == 4 and all(f.accepts(t)[0] == (t != 44) for t in gcc.TILES)
