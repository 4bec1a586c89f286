"""Which kernel v3d_gemm gives a call (v3d_amd/csrc/gemm.hip plan_gemm), checked on the CPU against what the library launched on an MI355X at
the commit before the planner existed: tests/golden/gemm_dispatch.json, written there by tools/record_gemm_dispatch.py (one U-Net evaluation,
VAE decode / encode, CLIP tower, scene size, frame-shard ranks, every GEMM case of tests/op_cases.py under the default and every forced
policy).  A kernel pull request that adds a branch to the planner sees here, without a GPU, that every other call still goes where it went.

The planner never dereferences a pointer, so the rows' pointers are rebuilt as synthetic addresses with the recorded alignment (mod 256)."""
import ctypes
import json
import os

import pytest

from v3d_amd.hip import _GemmArgs, c_vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "v3d_amd", "lib", "libv3d_hip.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lb = ctypes.CDLL(path)
    lb.v3d_debug_gemm_plan.restype = ctypes.c_int
    lb.v3d_debug_gemm_plan.argtypes = [ctypes.POINTER(_GemmArgs), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]
    return lb


def plan(lib, fx, row):
    cus, policy, ptr, val, _ = row
    a = _GemmArgs()
    for i, (name, mod) in enumerate(zip(fx["pointers"], ptr)):
        setattr(a, name, None if mod is None else ((i + 1) << 32) + mod)
    for name, v in zip(fx["values"], val):
        setattr(a, name, v)
    out = (ctypes.c_longlong * 10)()
    rc = lib.v3d_debug_gemm_plan(ctypes.byref(a), cus, (ctypes.c_int * 5)(*policy), out)
    assert rc == 0, f"the planner refuses arguments the library launched: {row}"
    return dict(zip(("kernel", "family", "bm", "bn", "tiles", "grid", "splitk", "streamk_tail", "gn_in_epilogue", "kernel_ids"), (int(v) for v in out)))


def test_fixture_names_the_argument_block():
    fx = json.load(open(FIXTURE))
    assert fx["pointers"] == [n for n, t in _GemmArgs._fields_ if t is c_vp] and fx["values"] == [n for n, t in _GemmArgs._fields_ if t is not c_vp]
    assert fx["knobs"] == ["V3D_GEMM_IMPL", "V3D_GEMM_SPLITK", "V3D_GEMM_V3S", "V3D_GEMM_V6", "V3D_STREAMK"]
    assert len({json.dumps(r[1]) for r in fx["rows"]}) == 8, "default policy + six forced settings of test_gemm_impls.py + V3D_STREAMK=0"


def test_every_recorded_call_gets_the_recorded_kernel(lib):
    """No row is left out, and the rows reach every kernel id of launch_plan's switch."""
    fx = json.load(open(FIXTURE))
    assert len(fx["rows"]) >= 300
    gn_stats = fx["pointers"].index("gn_stats")
    hit, wrong, ids = set(), [], None
    for row in fx["rows"]:
        family, bm, bn, tiles, splitk, tail, sk_launch, gn_launch = row[4]
        got = plan(lib, fx, row)
        ids = got["kernel_ids"]
        hit.add(got["kernel"])
        # the recorded GroupNorm counter counts v3 <GN> epilogues; the LDS-haloed kernels (family 5) gather gn_stats themselves whenever it is given
        gn = bool(gn_launch) or (family == 5 and row[2][gn_stats] is not None)
        want = dict(family=family, bm=bm, bn=bn, tiles=tiles, splitk=splitk, streamk_tail=tail, gn_in_epilogue=int(gn))
        assert bool(tail) == bool(sk_launch), f"fixture row contradicts itself: {row}"
        if {k: got[k] for k in want} != want:
            wrong.append((row, got))
    assert not wrong, f"{len(wrong)} of {len(fx['rows'])} calls would get another kernel, first: {wrong[0]}"
    assert hit == set(range(ids)), f"kernel ids no recorded call reaches: {sorted(set(range(ids)) - hit)} (add a shape to tools/record_gemm_dispatch.py)"


def test_plan_ignores_everything_but_alignment_of_pointers(lib):
    fx = json.load(open(FIXTURE))
    for row in fx["rows"][::25]:
        moved = [row[0], row[1], [None if m is None else m + 256 * 7 for m in row[2]], row[3], row[4]]
        assert plan(lib, fx, row) == plan(lib, fx, moved)
