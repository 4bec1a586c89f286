"""The mesh check without a GPU (include/v3d_recon.h "Mesh check", csrc_recon/meshcheck.hip, v3d_amd/recon/mesh_check.py,
scripts/pub/check_mesh.py): the scenes of tests/test_mesh_check_gpu.py keep their margin, the float32 and float64 restatements
(tests/mesh_check_ref.py) agree and the second formulation agrees with them, the prototype's counts are pinned, the census restatement
returns what is known of every census mesh, the library declares, exports and binds the four entries and refuses bad arguments before any
launch, the script refuses bad arguments before it imports the library, and the report's arithmetic holds on hand-fed kernel outputs."""
import importlib.util
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import mesh_check_ref as R
from v3d_amd.recon import mesh_check as MK                                      # (without the feature: the import fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_ENTRIES = {"v3d_recon_bvh_self_count", "v3d_recon_bvh_self_emit", "v3d_recon_mesh_edge_census", "v3d_recon_mesh_vertex_census"}


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PAIR_SCENES)
def test_scenes_keep_their_margin_and_both_precisions_agree(name):
    """A condition on the inputs: every decision of rule (d) on every scene stands SCENE_MARGIN away from its threshold, where the float32
    error of a plane distance at these sizes is about 1e-7.  An eroded scene fails here, not as a flaky GPU test."""
    o, o32 = R.oracle(name), R.oracle32(name)
    print(f"{name}: {len(o['pairs'])} pairs ({o['shared']} share a vertex) of {o['reached']} that reach (d); smallest margin {o['margin']:.3e}; "
          f"smallest relative |det| of the second formulation {o['min_det']:.3e}")
    assert o["margin"] >= R.SCENE_MARGIN, (name, o["margin"])
    assert o32["pairs"] == o["pairs"] and o32["reached"] == o["reached"]
    assert o["disagree"] == 0                              # Moeller-Trumbore agrees wherever its determinant is not small
    assert all(f < g for f, g in o["pairs"]) and o["pairs"] == sorted(set(o["pairs"]))
    if o["plane"].numel():
        assert float((o32["plane"].double() - o["plane"]).abs().max()) < 1e-5       # the float32 run follows the same statements


def test_the_prototypes_counts_are_pinned():
    for kind, (pairs, shared) in R.PINNED.items():
        got = [R.oracle(f"{kind}-{s}") for s in R.SEEDS]
        assert tuple(len(o["pairs"]) for o in got) == pairs, kind
        assert tuple(o["shared"] for o in got) == shared, kind
    assert [R.scene(f"{k}-1")[1].shape[0] for k in ("sphere", "pair", "fold")] == [320, 640, 320]
    assert R.scene("pair3")[1].shape[0] == 2553 and 2553 % 64 != 0
    assert len(R.oracle("pair3")["pairs"]) > 100
    # the quotient form is why rule (d) is plane-side first: on the sphere its determinant all but vanishes
    assert min(R.oracle(f"sphere-{s}")["min_det"] for s in R.SEEDS) < 1e-9


def test_cases_gives_exactly_the_expected_pairs():
    o = R.oracle("cases")
    assert o["pairs"] == R.CASES_PAIRS and o["shared"] == 1
    assert o["reached"] == 3                               # the two pairs and the pair that does not cross; nothing else gets past (a), (b), (c)
    v, f = R.scene("cases")
    assert R.candidates(v, f)[5] == len(R.CASES_FACES) - 3                          # absent, repeated index, no area
    assert R.oracle("single-1")["pairs"] == [] and R.oracle("single-2")["pairs"] == [(0, 1)]
    # the antipode without the offsets is degenerate: the margin collapses, which is why fold keeps them
    vv, ff = R.M.icosphere(2, 0.5, R.FOLD_CENTRE, 1)
    c = torch.tensor(R.FOLD_CENTRE, dtype=torch.float64)
    vd = vv.double()
    for i, _ in R.FOLD_MOVES:
        vd[i] = c - 1.3 * (vd[i] - c)
    assert R.pair_rule(vd.float(), ff)["margin"] < 1e-6


def test_edge_test_on_one_triangle():
    t = lambda *rows: torch.tensor(rows, dtype=torch.float64)  # noqa: E731
    a, b, c = t((0, 0, 0)), t((1, 0, 0)), t((0, 1, 0))
    for p, q, want in (((0.2, 0.2, 1), (0.2, 0.2, -1), True), ((0.2, 0.2, -1), (0.2, 0.2, 1), True), ((0.2, 0.2, 1), (0.2, 0.2, 0.5), False),
                       ((0.2, 0.2, 1), (0.2, 0.2, 0), False), ((2, 2, 1), (2, 2, -1), False), ((0, 0, 1), (0, 0, -1), True),
                       ((0.5, 0.5, 1), (0.5, 0.5, -1), True), ((-0.1, 0.5, 1), (-0.1, 0.5, -1), False), ((0, 0, 0), (1, 1, 0), False)):
        assert bool(R.edge_test(t(p), t(q), a, b, c)[0]) is want, (p, q)
        assert bool(R.edge_test(t(p), t(q), a, c, b)[0]) is want, (p, q)            # the other winding


# ---- the census -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CENSUS_MESHES)
def test_census_restatement_returns_the_known_figures(name):
    v, f = R.census_mesh(name)
    r = R.report(v, f)
    for k, want in R.CENSUS_FACTS[name].items():
        assert r[k] == want, (name, k, r[k], want)
    same, opposite, flags = R.census(f, v.shape[0])
    assert len(same) == len(opposite) == 3 * f.shape[0] and len(flags) == v.shape[0]
    if name == "icosphere":
        assert set(same) == set(opposite) == {1} and set(flags) == {0}
        # inscribed in the sphere of radius 0.5: below its volume and area, by a few per cent at 320 faces; positive: wound outwards
        assert 0.95 * (math.pi / 6) < r["volume"] < math.pi / 6 and 0.95 * math.pi < r["area"] < math.pi
    if name == "fin":
        assert (same[0], opposite[0]) == (2, 1) and (same[3], opposite[3]) == (1, 2) and flags[0] == flags[1] == R.OPEN | R.NON_MANIFOLD
    if name == "bow_tie":
        assert flags == [R.PINCHED] + [0] * 6
    if name == "flipped":
        assert sorted(zip(same, opposite)).count((2, 0)) == 6 and sum(1 for b in flags if b & R.WINDING) == 3
    if name == "cases":
        assert same[3 * 8:3 * 10] == [-1] * 6 and flags[17] & R.OPEN and (same[3 * 6], opposite[3 * 6]) == (2, 0)


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert CHECK_ENTRIES <= declared and declared == set(geometry.SIGNATURES)
    for name in CHECK_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1              # the new entries are additive
    assert int(re.search(r"#define V3D_RECON_ABI_VERSION (\d+)", hdr).group(1)) == 1
    assert "Mesh check" in hdr and "THE PAIR RULE" in hdr and "THE CENSUS" in hdr
    csrc = os.path.join(ROOT, "v3d_amd", "csrc_recon")
    src = open(os.path.join(csrc, "meshcheck.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")
    assert '#include "bvh_walk.h"' in src and '#include "mesh_lists.h"' in src
    assert "closed_fan(L," in src and "bool closed_fan(" not in src              # reused, not rewritten
    assert (MK.OPEN, MK.NON_MANIFOLD, MK.WINDING, MK.PINCHED) == (R.OPEN, R.NON_MANIFOLD, R.WINDING, R.PINCHED) == (1, 2, 4, 8)


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731
    tree = (p, p, p, p, p, p, 10, p, 4)
    assert lib.v3d_recon_bvh_self_count(*tree, None, p, None) == -1 and "v3d_recon_bvh_self_count" in err() and "null" in err()
    assert lib.v3d_recon_bvh_self_count(p, p, None, p, p, p, 10, p, 4, p, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_bvh_self_count(p, p, p, p, p, p, 0, p, 4, p, p, None) == -1 and "num_verts" in err()
    assert lib.v3d_recon_bvh_self_count(p, p, p, p, p, p, 10, p, 0, p, p, None) == -1 and "num_faces" in err()
    assert lib.v3d_recon_bvh_self_count(p, p, p, p, p, p, 10, p, 2 ** 30 + 1, p, p, None) == -1 and "num_faces" in err()
    assert lib.v3d_recon_bvh_self_emit(*tree, None, 1, p, None) == -1 and "v3d_recon_bvh_self_emit" in err() and "null" in err()
    assert lib.v3d_recon_bvh_self_emit(*tree, p, 1, None, None) == -1 and "null" in err()
    assert lib.v3d_recon_bvh_self_emit(*tree, p, 0, p, None) == -1 and "num_pairs" in err()
    assert lib.v3d_recon_mesh_edge_census(p, 4, p, p, 10, p, None, None) == -1 and "v3d_recon_mesh_edge_census" in err() and "null" in err()
    assert lib.v3d_recon_mesh_edge_census(p, 0, p, p, 10, p, p, None) == -1 and "num_faces" in err()
    assert lib.v3d_recon_mesh_edge_census(p, 2 ** 31 // 3 + 1, p, p, 10, p, p, None) == -1 and "INT32_MAX" in err()
    assert lib.v3d_recon_mesh_vertex_census(p, 4, p, None, 10, p, None) == -1 and "v3d_recon_mesh_vertex_census" in err() and "null" in err()
    assert lib.v3d_recon_mesh_vertex_census(p, 4, p, p, 0, p, None) == -1 and "num_verts" in err()


def test_host_api_refuses_bad_arguments_with_its_name():
    v, f = R.scene("cases")
    with pytest.raises(ValueError, match="self_intersections"):
        MK.self_intersections("not a tree")
    for bad in (0, -1, 2 ** 31, 2.5, True, None):
        with pytest.raises(ValueError, match="self_intersections: max_pairs"):
            MK.self_intersections(_tree_on_the_host(v, f), bad)
        with pytest.raises(ValueError, match="check_mesh: max_pairs"):
            MK.check_mesh(v, f, device="cpu", max_pairs=bad)
    for bv, bf in ((v[:, :2], f), (v, f[:, :2]), (v, f.float()), (v[:0], f), (v, f[:0]), (torch.full_like(v, float("nan")), f)):
        with pytest.raises(ValueError, match="check_mesh"):
            MK.check_mesh(bv, bf, device="cpu")
    for bf, bn in ((f.float(), 29), (f[:, :2], 29), (f[:0], 29), (f, 0), (f, -3), (f, 2.5), (f, 2 ** 31)):
        with pytest.raises(ValueError, match="edge_census"):
            MK.edge_census(bf, bn, device="cpu")


def _tree_on_the_host(v, f):
    """a MeshBVH that no entry may ever receive: the argument checks come first"""
    from v3d_amd.recon.mesh_bake import MeshBVH
    z = torch.zeros(1, dtype=torch.int32)
    return MeshBVH(v, f.int(), z, z, z, z, torch.zeros(1, 3), torch.zeros(1, 3), 0)


# ---- the script -----------------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_check_mesh_options_parse_and_are_checked_before_the_library_is_imported(monkeypatch):
    mod = _entry("check_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh_50k.ply"]))
    assert a == {"mesh": "out/gs/mesh_50k.ply", "json": None, "paint": None, "max_pairs": 1 << 24, "strict": False}
    b = vars(ap.parse_args(["--mesh", "m.obj", "--json", "r.json", "--paint", "p.ply", "--strict", "--max_pairs", "10"]))
    assert (b["json"], b["paint"], b["strict"], b["max_pairs"]) == ("r.json", "p.ply", True, 10)
    with pytest.raises(SystemExit):
        ap.parse_args([])
    # (a bad argument must end the run before main's imports, render_mesh first and the library after it, are reached: the poisoned module
    # would raise ImportError instead)
    monkeypatch.setitem(sys.modules, "render_mesh", None)
    base = ["--mesh", "does/not/exist.ply"]
    for bad in (["--json", "out.txt"], ["--paint", "out.obj"], ["--paint", "does/not/exist.ply"], ["--max_pairs", "0"], ["--max_pairs", str(2 ** 31)]):
        with pytest.raises(SystemExit):
            mod.main(base + bad)
    with pytest.raises(SystemExit):
        mod.main(["--mesh", "does/not/exist.glb"])
    with pytest.raises(ImportError):                       # good arguments do reach the import
        mod.main(base)


def test_paint_colours():
    mod = _entry("check_mesh")
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 9]])
    c = mod.paint_colors(7, faces, np.array([0, 2, 1]), np.array([MK.OPEN, 0, MK.OPEN | MK.NON_MANIFOLD, MK.OPEN, 0, 0, MK.PINCHED]))
    want = [mod.BOUNDARY, mod.GREY, mod.INTERSECTING, mod.INTERSECTING, mod.INTERSECTING, mod.INTERSECTING, mod.GREY]
    assert np.array_equal(c, np.asarray(want, dtype=np.float32))
    assert len({mod.GREY, mod.INTERSECTING, mod.NON_MANIFOLD, mod.BOUNDARY}) == 4


# ---- the report's arithmetic, on hand-fed kernel outputs ----------------------------------------------------------------------------------
def _fed(name):
    """build_report on the restatement's census in the place of the kernels' outputs"""
    v, f = R.census_mesh(name)
    same, opposite, flags = R.census(f, v.shape[0])
    o = R.pair_rule(v, f)
    return MK.build_report(v, f, same, opposite, flags, R.components(f, v.shape[0]), R.degrees(o["pairs"], f.shape[0]), len(o["pairs"]), 0.25)


@pytest.mark.parametrize("name", R.CENSUS_MESHES)
def test_report_arithmetic_on_hand_fed_outputs(name):
    r = _fed(name)
    assert R.same_report(r, R.report(*R.census_mesh(name)))
    assert r["seconds"] == 0.25 and set(r) == set(R.report(*R.census_mesh(name))) | {"seconds"}
    for k, want in R.CENSUS_FACTS[name].items():
        assert r[k] == want, (name, k)
    assert all(type(x) in (int, float, bool, dict, type(None)) for x in r.values())


def test_report_of_a_tetrahedron_by_hand():
    v = torch.tensor([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (5.0, 5.0, 5.0)])
    f = torch.tensor([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)])
    ones = [1] * 12
    r = MK.build_report(v, f, ones, ones, [0] * 5, 1, [0] * 4, 0)
    assert (r["vertices"], r["vertices_used"], r["edges"], r["edges_by_multiplicity"], r["euler"], r["genus"]) == (5, 4, 6, {"2": 6}, 2, 0)
    assert r["watertight"] and abs(r["volume"] - 1 / 6) < 1e-15 and abs(r["area"] - (1.5 + math.sqrt(3) / 2)) < 1e-15
    # five faces' corners: 3 half-edges of multiplicity 1 are 3 edges; two that run the same way are one edge; 9 of multiplicity 3 are 3; one
    # corner that is not counted
    same = [1, 1, 1, 2, 2, 3, 2, 1, 3, 2, 1, 3, 2, 1, -1]
    opposite = [0, 0, 0, 0, 0, 0, 1, 2, 0, 1, 2, 0, 1, 2, -1]
    r = MK.build_report(v, torch.cat([f, f[:1]]), same, opposite, [0] * 5, 1, [1, 1, 0, 0, 0], 1)
    assert r["edges_by_multiplicity"] == {"1": 3, "2": 1, "3": 3} and r["inconsistent_edges"] == 1 and r["non_manifold_edges"] == 3
    assert r["boundary_edges"] == 3 and not r["closed"] and not r["watertight"] and r["genus"] is None and r["volume"] is None
    assert (r["self_intersections"], r["intersecting_faces"]) == (1, 2)
    with pytest.raises(RuntimeError, match="multiplicity"):
        MK.build_report(v, f, [2] * 11 + [1], [1] * 12, [0] * 5, 1, [0] * 4, 0)   # 11 half-edges of multiplicity 3
