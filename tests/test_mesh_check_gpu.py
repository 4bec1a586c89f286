"""The gfx950 mesh check (csrc_recon/meshcheck.hip, v3d_amd/recon/mesh_check.py, scripts/pub/check_mesh.py) against the restatement
(tests/mesh_check_ref.py): the list of intersecting pairs equals the float64 brute force's exactly, with no tolerance and no exclusions
(tests/test_mesh_check_cpu.py holds every scene to a margin that makes this a fair demand of float32), the per-face counts are the degrees
of that list, the raw entries write nothing outside their outputs and two runs are bit-equal, the census equals the dicts' on every census
mesh, the report equals the restated report, and the script writes what it says."""
import functools
import importlib.util
import json
import os
import time

import numpy as np
import pytest
import torch

import mesh_check_ref as R
import mesh_render_ref as M
from conftest import record_parity
from v3d_amd.ops import get_ops
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_bake as MB
from v3d_amd.recon import mesh_check as MK
from v3d_amd.recon import mesh_clean as MC
from v3d_amd.recon import mesh_decimate as MD

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096


@functools.lru_cache(maxsize=None)
def scene_bvh(name):
    return MB.build_bvh(*R.scene(name))


class Guarded:
    """An output of n rows with GUARD sentinel elements before and after it (the pattern of tests/test_mesh_query_gpu.py)"""

    def __init__(self, n, width, dtype, sentinel):
        self.n, self.width, self.sentinel = n, width, sentinel
        self.buf = torch.full((2 * GUARD + n * width,), sentinel, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def take(self):
        assert bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.n * self.width:] == self.sentinel).all()), "a guard was written"
        out = self.buf[GUARD:GUARD + self.n * self.width]
        return (out.reshape(self.n, self.width) if self.width > 1 else out).clone()


# ---- 1. the pairs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PAIR_SCENES)
def test_pairs_are_exactly_the_brute_forces(name):
    o, o32 = R.oracle(name), R.oracle32(name)
    F = R.scene(name)[1].shape[0]
    bvh = scene_bvh(name)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = MK.self_intersections(bvh)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    pairs = got["pairs"].cpu()
    plane_err = float((o32["plane"].double() - o["plane"]).abs().max()) if o["plane"].numel() else 0.0
    bary_err = float((o32["bary"].double() - o["bary"]).abs().max()) if o["bary"].numel() else 0.0
    print(f"{name}: F {F}: {got['count']} pairs (brute force {len(o['pairs'])}), smallest margin {o['margin']:.3e}; float32 restatement off by "
          f"{plane_err:.3e} in plane distance, {bary_err:.3e} in barycentrics; {seconds:.4f} s")
    record_parity(f"mesh_check_pairs[{name}]", {"faces": F, "pairs": got["count"], "smallest_margin": o["margin"] if o["reached"] else None,
                                                "float32_plane_distance_max_abs": plane_err, "float32_barycentric_max_abs": bary_err, "seconds": seconds})
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (len(o["pairs"]), 2) and got["count"] == len(o["pairs"])
    assert [tuple(p) for p in pairs.tolist()] == o["pairs"]                         # set equality and the order, no tolerance, no exclusions
    assert got["per_face"].dtype == torch.int32 and got["per_face"].cpu().tolist() == R.degrees(o["pairs"], F)
    again = MK.self_intersections(bvh)
    assert torch.equal(again["pairs"], got["pairs"]) and torch.equal(again["per_face"], got["per_face"]), "two runs differ"


@pytest.mark.parametrize("name", ("pair-1", "fold-2", "cases", "pair3", "single-1", "single-2"))
def test_raw_entries_stay_inside_their_outputs(name):
    o = R.oracle(name)
    bvh = scene_bvh(name)
    F = bvh.num_faces
    lib = G.load_library()
    runs = []
    for _ in range(2):
        n_all, n_up = Guarded(F, 1, torch.int32, -7), Guarded(F, 1, torch.int32, -7)
        G._check(lib, lib.v3d_recon_bvh_self_count(*bvh._args(), n_all.ptr, n_up.ptr, G._stream()), "self_count")
        n_all, n_up = n_all.take(), n_up.take()
        assert n_all.cpu().tolist() == R.degrees(o["pairs"], F)
        assert n_up.cpu().tolist() == [sum(1 for p in o["pairs"] if p[0] == f) for f in range(F)]
        total = int(n_up.sum())
        assert total == len(o["pairs"])
        offsets = get_ops().gs_scan(n_up)
        pairs = Guarded(max(total, 1), 2, torch.int32, -7)
        G._check(lib, lib.v3d_recon_bvh_self_emit(*bvh._args(), offsets.data_ptr(), max(total, 1), pairs.ptr, G._stream()), "self_emit")
        pairs = pairs.take()[:total]
        runs.append((n_all, n_up, pairs))
        rows = pairs.cpu().tolist()
        assert [r[0] for r in rows] == sorted(r[0] for r in rows)                    # grouped by f, ascending
        assert sorted(tuple(r) for r in rows) == o["pairs"]
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ"
    if total > 1:
        # a buffer shorter than the list: filled to its end and no further
        short = Guarded(total - 1, 2, torch.int32, -7)
        G._check(lib, lib.v3d_recon_bvh_self_emit(*bvh._args(), offsets.data_ptr(), total - 1, short.ptr, G._stream()), "self_emit")
        assert torch.equal(short.take(), runs[0][2][:total - 1])


def test_more_pairs_than_max_pairs_are_counted_and_not_listed():
    o = R.oracle("pair-1")
    got = MK.self_intersections(scene_bvh("pair-1"), max_pairs=10)
    assert got["pairs"] is None and got["count"] == len(o["pairs"]) == 76
    assert got["per_face"].cpu().tolist() == R.degrees(o["pairs"], 640)
    exact = MK.self_intersections(scene_bvh("pair-1"), max_pairs=76)
    assert exact["pairs"] is not None and exact["pairs"].shape[0] == 76
    timings = {}
    MK.self_intersections(scene_bvh("pair-1"), timings=timings)
    assert set(timings) == {"count", "scan", "emit", "sort"} and all(t >= 0 for t in timings.values())


# ---- 2. the census --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CENSUS_MESHES)
def test_census_and_report_equal_the_restatement(name):
    v, f = R.census_mesh(name)
    V, F = v.shape[0], f.shape[0]
    same, opposite, flags = MK.edge_census(f, V)
    want = R.census(f, V)
    assert same.dtype == opposite.dtype == flags.dtype == torch.int32
    assert (same.cpu().tolist(), opposite.cpu().tolist(), flags.cpu().tolist()) == want
    # the raw entries, guarded
    lib = G.load_library()
    fd = f.clamp(-1, 2 ** 31 - 1).to(DEV, torch.int32).contiguous()
    ranges, corners = MC._corner_lists(fd, V)
    gs, go, gf = Guarded(3 * F, 1, torch.int32, -7), Guarded(3 * F, 1, torch.int32, -7), Guarded(V, 1, torch.int32, -7)
    G._check(lib, lib.v3d_recon_mesh_edge_census(fd.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, gs.ptr, go.ptr, G._stream()), "edge_census")
    G._check(lib, lib.v3d_recon_mesh_vertex_census(fd.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, gf.ptr, G._stream()), "vertex_census")
    assert torch.equal(gs.take(), same) and torch.equal(go.take(), opposite) and torch.equal(gf.take(), flags)
    r = MK.check_mesh(v, f)
    ref = R.report(v, f)
    print(f"{name}: {r}")
    assert R.same_report(r, ref) and set(r) == set(ref) | {"seconds"} and r["seconds"] > 0
    for k, x in R.CENSUS_FACTS[name].items():
        assert r[k] == x, (name, k)
    record_parity(f"mesh_check_report[{name}]", {k: r[k] for k in ("faces", "edges", "euler", "genus", "self_intersections", "watertight", "seconds")})


def test_check_mesh_of_the_icosphere_and_of_the_pair():
    v, f = R.census_mesh("icosphere")
    r = MK.check_mesh(v, f)
    a, b, c = (v.double()[f[:, k]] for k in range(3))
    volume = float((a * torch.linalg.cross(b, c)).sum()) / 6.0                       # both in torch float64
    assert r["watertight"] and r["genus"] == 0 and abs(r["volume"] - volume) <= 1e-12 * abs(volume) and r["volume"] > 0
    assert (r["closed"], r["manifold"], r["oriented"], r["components"], r["euler"]) == (True, True, True, 1, 2)
    r = MK.check_mesh(*R.scene("pair-1"))
    assert (r["closed"], r["manifold"], r["oriented"], r["components"], r["watertight"]) == (True, True, True, 2, False)
    assert r["self_intersections"] == 76 and r["genus"] == 0
    report, d = MK.check_mesh(*R.scene("fold-1"), details=True)
    assert set(d) == {"pairs", "per_face", "same", "opposite", "flags"} and d["pairs"].shape[0] == report["self_intersections"] == 69
    assert report["closed"] and report["manifold"] and report["oriented"] and not report["watertight"]


def test_argument_errors_come_before_any_launch():
    v, f = R.scene("cases")
    bvh = scene_bvh("cases")
    for bad in (0, -1, 2 ** 31, 2.5, True):
        with pytest.raises(ValueError, match="self_intersections: max_pairs"):
            MK.self_intersections(bvh, bad)
        with pytest.raises(ValueError, match="check_mesh: max_pairs"):
            MK.check_mesh(v, f, max_pairs=bad)
    with pytest.raises(ValueError, match="self_intersections"):
        MK.self_intersections((v, f))
    with pytest.raises(ValueError, match="check_mesh"):
        MK.check_mesh(v, f.float())
    with pytest.raises(ValueError, match="check_mesh"):
        MK.check_mesh(v, f[:0])
    with pytest.raises(ValueError, match="edge_census"):
        MK.edge_census(f, 0)
    with pytest.raises(ValueError, match="edge_census"):
        MK.edge_census(f[:0], 29)


# ---- 3. the script and the stage before it --------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_check_mesh_script_end_to_end(tmp_path, capsys):
    mod = _entry("check_mesh")
    v, f = R.scene("fold-1")
    grey = np.full((v.shape[0], 3), 0.5, dtype=np.float32)
    fold, sphere = str(tmp_path / "fold.ply"), str(tmp_path / "sphere.ply")
    G.save_mesh_ply(fold, v, f, grey)
    G.save_mesh_ply(sphere, *R.scene("sphere-1"), grey)
    out_json, out_ply = str(tmp_path / "fold_check.json"), str(tmp_path / "fold_check.ply")
    mod.main(["--mesh", fold, "--json", out_json, "--paint", out_ply])                # a plain run exits 0 whatever it finds
    out = capsys.readouterr().out
    assert out.count("\n") == 3 and "NOT watertight" in out and "69 intersecting pairs" in out
    r = json.load(open(out_json))
    assert R.same_report(r, R.report(v, f)) and r["mesh"] == fold and not r["watertight"]
    pv, pf, pc = G.read_mesh_ply(out_ply)
    assert np.array_equal(pv, v.numpy()) and np.array_equal(pf, f.numpy())
    marked = {i for p in R.oracle("fold-1")["pairs"] for k in p for i in f[k].tolist()}
    red = tuple(int(round(255 * x)) for x in mod.INTERSECTING)
    assert {i for i in range(v.shape[0]) if tuple(pc[i]) == red} == marked           # exactly the vertices of the faces in the list
    assert {tuple(c) for i, c in enumerate(pc.tolist()) if i not in marked} == {tuple(int(round(255 * x)) for x in mod.GREY)}
    with pytest.raises(SystemExit) as e:
        mod.main(["--mesh", fold, "--strict"])
    assert e.value.code == 1
    mod.main(["--mesh", sphere, "--strict"])                                         # returns: status 0
    assert ": watertight;" in capsys.readouterr().out.splitlines()[-1]


def test_the_report_of_a_decimated_sphere_is_the_restatements():
    """Not a promise about decimate_mesh: whatever it leaves behind, the kernels and the restatement must say the same of it"""
    v, f = M.icosphere(3, 0.5, (0.0, 0.0, 0.0), 1)
    assert f.shape[0] == 1280
    dv, df, _, stats = MD.decimate_mesh(v, f, None, 400)
    dv, df = dv.cpu(), df.cpu().long()
    r = MK.check_mesh(dv, df)
    print(f"decimated to {df.shape[0]} faces ({stats['stopped']}): {r}")
    assert R.same_report(r, R.report(dv, df))
    hits = MK.self_intersections(MB.build_bvh(dv, df))
    assert [tuple(p) for p in hits["pairs"].cpu().tolist()] == R.pair_rule(dv, df)["pairs"]
    record_parity("mesh_check_downstream[decimate-1280-400]", {k: r[k] for k in ("faces", "vertices_used", "edges", "euler", "genus", "boundary_edges",
                                                                                 "non_manifold_edges", "self_intersections", "watertight")})
