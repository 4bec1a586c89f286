"""The mesh repair without a GPU (include/v3d_recon.h "Mesh repair", csrc_recon/meshrepair.hip, v3d_amd/recon/mesh_repair.py,
scripts/pub/repair_mesh.py): the library declares, exports and binds the fifteen entries and refuses bad arguments before any launch, the
host functions and the script refuse theirs before anything is loaded, the restatement (tests/mesh_repair_ref.py) reproduces the prototype's
figures, and every scene that tests/test_mesh_repair_gpu.py compares exactly keeps SCENE_MARGIN in every check of every round."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import mesh_check_ref as R
import mesh_repair_ref as P
from v3d_amd.recon import mesh_repair as MR                                     # (without the feature: the import fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPAIR_ENTRIES = {"v3d_recon_repair_" + n for n in ("weld_keys", "weld_heads", "weld_first", "weld_remap", "remap_faces", "drop_flags", "orient_round",
                                                    "orient_conflicts", "orient_apply", "vertex_open", "trouble", "grow", "loop_round", "loop_flags",
                                                    "fill_emit")}
# what the restatement says of every scene: rounds, faces, vertices, watertight, components, why the loop stopped
PINNED = {
    "fold-1[grow_times=1]": (1, 264, 134, True, 1, "clean"), "fold-2[grow_times=1]": (1, 262, 133, True, 1, "clean"),
    "fold-3[grow_times=1]": (1, 258, 131, True, 1, "clean"), "fold-1[grow_times=2]": (1, 186, 95, True, 1, "clean"),
    "fold-2[grow_times=2]": (1, 172, 88, True, 1, "clean"), "fold-3[grow_times=2]": (1, 174, 89, True, 1, "clean"),
    "star-12": (1, 320, 162, True, 1, "clean"), "star-29": (1, 320, 162, True, 1, "clean"), "star-72": (1, 320, 162, True, 1, "clean"),
    "star-100": (1, 320, 162, True, 1, "clean"), "star-150": (1, 320, 162, True, 1, "clean"),
    "two-0_1": (1, 308, 156, True, 1, "clean"), "two-37_36": (1, 308, 156, True, 1, "clean"), "two-74_69": (1, 308, 156, True, 1, "clean"),
    "two-148_24": (1, 310, 157, True, 1, "clean"),
    "soup": (0, 320, 162, True, 1, "clean"), "mixed": (0, 320, 162, True, 1, "clean"), "inside_out": (0, 320, 162, True, 1, "clean"),
    "flipped_soup": (0, 320, 162, True, 1, "clean"), "icosphere": (0, 320, 162, True, 1, "clean"),
    "fin": (0, 3, 5, False, 1, "empty"), "bow_tie": (0, 8, 7, False, 1, "empty"), "cases": (1, 8, 11, False, 3, "stalled"),
    "open_grid[max_hole_edges=8]": (0, 30, 24, False, 1, "clean"),
    "pair-1": (2, 388, 200, True, 3, "clean"), "fold-1[grow_times=0]": (2, 318, 161, True, 1, "clean"), "open_grid": (1, 46, 25, False, 1, "empty"),
    "moebius": (1, 34, 19, True, 1, "clean"),
}
# the prototype's smallest margin of the final check, fold-1/2/3 at grow 1 and 2 (it took the centre in loop order: the last digits may differ)
PROTOTYPE_MARGINS = {"fold-1[grow_times=1]": 9.8e-4, "fold-2[grow_times=1]": 1.06e-4, "fold-3[grow_times=1]": 4.1e-4,
                     "fold-1[grow_times=2]": 2.7e-4, "fold-2[grow_times=2]": 9.5e-4, "fold-3[grow_times=2]": 1.03e-4}


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", P.MARGIN_SCENES + P.PLAIN_SCENES, ids=[P.key_of(n, k) for n, k in P.MARGIN_SCENES + P.PLAIN_SCENES])
def test_every_check_of_every_round_keeps_the_margin(name, kw):
    """A condition on the inputs: the float32 kernels are held to this float64 restatement exactly, which is fair only where every decision
    of the pair rule, in every round, stands SCENE_MARGIN away from its threshold."""
    r = P.restated(name, kw)
    a = r["after"]
    print(f"{P.key_of(name, kw)}: {len(r['history'])} rounds, {len(r['faces'])} faces, watertight {a['watertight']}, stopped {r['stopped']}; margins "
          + " ".join(f"{m:.3e}" for m in r["margins"]))
    assert min(r["margins"]) >= R.SCENE_MARGIN, (name, r["margins"])
    assert (len(r["history"]), len(r["faces"]), len(r["verts"]), a["watertight"], a["components"], r["stopped"]) == PINNED[P.key_of(name, kw)]
    want = PROTOTYPE_MARGINS.get(P.key_of(name, kw))
    if want is not None:
        assert abs(r["margins"][1] - want) <= 0.02 * want and a["genus"] == 0
    for h in r["history"]:
        assert h["faces_after"] == h["faces"] - h["faces_cut"] + h["faces_filled"] - h["faces_dropped"]


@pytest.mark.parametrize("name,kw", P.WEAK_SCENES, ids=[P.key_of(n, k) for n, k in P.WEAK_SCENES])
def test_the_scenes_that_do_not_keep_the_margin_are_known(name, kw):
    r = P.restated(name, kw)
    assert min(r["margins"]) < R.SCENE_MARGIN                                    # which is why the GPU test asks less of them
    a = r["after"]
    assert (len(r["history"]), len(r["faces"]), len(r["verts"]), a["watertight"], a["components"], r["stopped"]) == PINNED[P.key_of(name, kw)]


def test_the_holes_are_what_the_issue_says():
    v, f = P.icosphere()
    for x in (12, 29, 72, 100, 150):
        assert sum(1 for r in f if x in r) == 6                                   # six-valent
    for a, b in ((0, 1), (37, 36), (74, 69), (148, 24)):
        assert len(set(f[a]) & set(f[b])) == 1                                    # the two faces share a vertex and nothing else
        r = P.restated(f"two-{a}_{b}", {})["history"][0]
        assert (r["bad_vertices"], r["pairs"], r["loops_filled"]) == (1, 0, 1)
    assert [P.restated(f"star-{x}", {})["history"][0]["faces_filled"] for x in (12, 29)] == [6, 6]


def _triangles(v, f):
    """the faces as positions: what a renumbering of the vertices leaves alone"""
    return [tuple(tuple(float(x) for x in v[i]) for i in r) for r in f]


def test_weld_orient_and_volume_on_the_plain_scenes():
    v0, f0 = P.icosphere()
    sv, sf = P.named("soup")
    assert sv.shape[0] == 960 and len(set(P.weld(sv))) == 162
    r = P.restated("soup", {})
    assert _triangles(r["verts"], r["faces"]) == _triangles(v0, f0) and r["verts"].shape[0] == 162 and r["after"]["watertight"]
    assert P.restated("mixed", {})["faces"] == f0 and P.named("mixed")[1] != f0
    assert sum(1 for a, b in zip(P.named("mixed")[1], f0) if a != b) > 60
    r = P.restated("inside_out", {})
    assert r["orient"]["flipped_patches"] == 1 and r["faces"] == f0 and r["after"]["volume"] > 0
    mv, mf = P.named("moebius")
    g, info = P.orient(mv, mf)
    assert info["non_orientable"] == 1 and g == mf                                 # counted, and left as it is
    rep = P.report(mv, mf)
    assert rep["boundary_edges"] == 24 and rep["components"] == 1 and not rep["oriented"]
    r = P.restated("flipped_soup", {})
    cv, cf = R.M.icosphere(2, 0.5, (0.0, 0.0, 0.0), 1)                             # (`flipped` stands at the origin)
    assert _triangles(r["verts"], r["faces"]) == _triangles(cv.numpy(), P.rows_of(cf)) and r["verts"].shape[0] == 162
    r = P.restated("icosphere", {})
    assert r["history"] == [] and r["faces"] == f0 and r["verts"].tobytes() == v0.tobytes()
    r = P.restated("open_grid", {"max_hole_edges": 8})
    assert r["history"] == [] and r["loops_left"] == 1 and r["faces"] == P.named("open_grid")[1]
    for name in ("fin", "bow_tie"):                                                # a round that would leave nothing: the state before it
        r = P.restated(name, {})
        assert r["stopped"] == "empty" and r["history"] == [] and r["faces"] == P.named(name)[1]


def test_weld_compares_by_value():
    v = np.array([(0.0, 1.0, 2.0), (-0.0, 1.0, 2.0), (0.0, 1.0, np.float32(2.0) + np.float32(2.4e-7)), (0.0, 1.0, 2.0), (5.0, -0.0, 0.0), (5.0, 0.0, -0.0)],
                 dtype=np.float32)
    assert P.weld(v) == [0, 0, 2, 0, 4, 4]
    assert P.drop_bits(v, [(0, 2, 4), (4, 0, 2), (0, 0, 4), (0, 2, 9), (2, 4, 0), (0, 2, 2)]) == [0, 8, 6, 1, 8, 6]


def test_pass_restatements_on_hand_built_loops():
    # two triangles' worth of open half-edges: 0 -> 2 -> 4 -> 0 and 1 -> 3 -> 5 -> 7 -> 1 interleave; 6 is a dead end into bad 8
    nxt = [2, 3, 4, 5, 0, 7, 8, 1, -1]
    bad = [0, 0, 0, 0, 0, 0, 0, 0, 1]
    lab, jump = P.loop_labels(bad, nxt)
    assert lab[:6] == [0, 1, 0, 1, 0, 1] and jump[6] == -1 and jump[8] == -1
    state, length, members = P.loop_flags(bad, nxt, lab, jump, 4)
    assert state == [1, 1, 0, 0, 0, 0, 0, 0, 0] and length[:2] == [3, 4] and members == {0: [0, 2, 4], 1: [1, 3, 5, 7]}
    assert P.loop_flags(bad, nxt, lab, jump, 3)[0][:2] == [1, 2]                   # one edge too long
    v = np.arange(27, dtype=np.float32).reshape(9, 3)
    faces, nv, nc = P.fill_emit(v, None, nxt, state, length, members)
    assert faces == [(4, 2, 0), (3, 1, 9), (5, 3, 9), (7, 5, 9), (1, 7, 9)] and nc is None
    assert np.array_equal(nv, np.array([[(3 + 9 + 15 + 21) / 4, (4 + 10 + 16 + 22) / 4, (5 + 11 + 17 + 23) / 4]], dtype=np.float32))
    # a chain that runs into a loop: with the smaller index it is a class of its own and the loop is filled; with a larger one it shares the
    # loop's label, the rows no longer close, and the loop is left
    for nxt2, want in (([1, 2, 3, 1], [2, 1, 0, 0]), ([1, 2, 0, 0], [2, 0, 0, 0])):
        lab2, jump2 = P.loop_labels([0] * 4, nxt2)
        assert P.loop_flags([0] * 4, nxt2, lab2, jump2, 10)[0] == want


def test_patch_flips_of_the_host_module_follow_the_restatement():
    v, f = P.named("inside_out")
    same, opposite, _ = R.census(f, v.shape[0])
    lab, _ = P.orient_labels(f, v.shape[0], same, opposite)
    marks = P.orient_conflicts(f, v.shape[0], same, opposite, lab)
    flip = MR.patch_flips(v, np.asarray(f), np.asarray(lab), np.asarray(same), np.asarray(opposite), np.asarray(marks))
    assert flip.tolist() == [1] + [0] * 319 and flip.dtype == np.int32
    gv, gf = P.named("open_grid")                                                  # an open patch keeps the winding of its lowest face
    gf = [(r[0], r[2], r[1]) for r in gf]
    same, opposite, _ = R.census(gf, gv.shape[0])
    lab, _ = P.orient_labels(gf, gv.shape[0], same, opposite)
    assert not MR.patch_flips(gv, np.asarray(gf), np.asarray(lab), np.asarray(same), np.asarray(opposite), np.zeros(len(gf), dtype=np.int32)).any()


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert len(REPAIR_ENTRIES) == 15 and REPAIR_ENTRIES <= declared and declared == set(geometry.SIGNATURES)
    for name in REPAIR_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1              # the new entries are additive
    assert int(re.search(r"#define V3D_RECON_ABI_VERSION (\d+)", hdr).group(1)) == 1
    assert "Mesh repair" in hdr and all(w in hdr for w in ("WELD.", "DROP.", "ORIENT.", "CUT.", "FILL."))
    csrc = os.path.join(ROOT, "v3d_amd", "csrc_recon")
    src = open(os.path.join(csrc, "meshrepair.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")
    assert '#include "bvh_walk.h"' in src and '#include "mesh_lists.h"' in src
    for reused in ("struct Lists {", "bool load_face(", "bool closed_fan(", "bool no_area("):      # reused, not rewritten
        assert reused not in src
    assert "no_area(" in src and "load_face(" in src and "const Lists&" in src
    assert (MR.ABSENT, MR.REPEATED, MR.NO_AREA, MR.DUPLICATE, MR.DOUBLING_ROUNDS) == (1, 2, 4, 8, P.DOUBLING_ROUNDS)


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p, big = 0x1000, 2 ** 31 // 3 + 1
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731

    def refused(name, args, word):
        assert getattr(lib, "v3d_recon_repair_" + name)(*args, None) == -1, name
        assert "v3d_recon_repair_" + name in err() and word in err(), (name, err())

    refused("weld_keys", (p, 5, None, p, p), "null")
    refused("weld_keys", (p, 0, p, p, p), "num_verts")
    refused("weld_heads", (p, 5, p, None), "null")
    refused("weld_heads", (p, -1, p, p), "num_verts")
    refused("weld_first", (p, p, None, 5, p), "null")
    refused("weld_first", (p, p, p, 0, p), "num_verts")
    refused("weld_remap", (None, p, p, 5, p), "null")
    refused("weld_remap", (p, p, p, 0, p), "num_verts")
    refused("remap_faces", (p, 4, 5, p, None), "null")
    refused("remap_faces", (p, 4, 5, p, p), "two buffers")
    refused("remap_faces", (p, 0, 5, p, p + 64), "num_faces")
    refused("drop_flags", (p, 5, p, 4, p, p, None), "null")
    refused("drop_flags", (p, 5, p, big, p, p, p), "INT32_MAX")
    refused("orient_round", (p, 4, p, p, 5, p, p, p, None, p), "null")
    refused("orient_round", (p, 4, p, p, 5, p, p, p, p, p), "two buffers")
    refused("orient_round", (p, 0, p, p, 5, p, p, p, p + 64, p), "num_faces")
    refused("orient_conflicts", (p, 4, p, p, 5, p, p, p, None), "null")
    refused("orient_conflicts", (p, 4, p, p, 0, p, p, p, p), "num_verts")
    refused("orient_apply", (p, 4, p, None, None, p + 64), "null")
    refused("orient_apply", (p, 4, p, p, None, p), "two buffers")
    refused("orient_apply", (p, 0, p, p, None, p + 64), "num_faces")
    refused("vertex_open", (p, 4, p, p, 5, p, p, p, p, None), "null")
    refused("vertex_open", (p, 4, p, p, 0, p, p, p, p, p), "num_verts")
    refused("trouble", (p, 4, 5, p, None, p), "null")
    refused("trouble", (p, 0, 5, p, p, p), "num_faces")
    refused("grow", (p, 4, p, p, 5, p, p), "two buffers")
    refused("grow", (p, 4, p, p, 5, None, p), "null")
    refused("loop_round", (5, p, p, p, p + 64), "two buffers")
    refused("loop_round", (5, p, None, p + 64, p + 128), "null")
    refused("loop_round", (0, p, p + 64, p + 128, p + 192), "num_verts")
    refused("loop_flags", (5, p, p, p, p, p, p, 2, p, p), "max_hole_edges")
    refused("loop_flags", (5, p, p, p, p, p, None, 3, p, p), "null")
    refused("fill_emit", (p, None, 5, p, p, p, p, p, p, p, 0, 0, p, None, None), "new faces")
    refused("fill_emit", (p, None, 5, p, p, p, p, p, p, p, 4, 1, p, None, None), "null output")
    refused("fill_emit", (p, p, 5, p, p, p, p, p, p, p, 4, 1, p, p, None), "null output")
    refused("fill_emit", (p, None, 2 ** 31 - 1, p, p, p, p, p, p, p, 4, 1, p, p, None), "INT32_MAX")
    refused("fill_emit", (p, None, 5, p, p, p, p, p, p, None, 4, 0, p, None, None), "null")


def test_host_api_refuses_bad_arguments_with_its_name():
    v, f = R.scene("cases")
    for kw in ({"grow": -1}, {"grow": 2.5}, {"grow": True}, {"max_rounds": -1}, {"max_rounds": None}, {"max_hole_edges": 2}, {"max_hole_edges": 2.5},
               {"orient": 1}, {"weld": "yes"}):
        with pytest.raises(ValueError, match="repair_mesh: " + next(iter(kw))):
            MR.repair_mesh(v, f, device="cpu", **kw)
    nan = torch.full_like(v, float("nan"))
    for bv, bf, bc in ((v[:, :2], f, None), (v, f[:, :2], None), (v, f.float(), None), (v[:0], f, None), (v, f[:0], None), (nan, f, None),
                       (torch.where(torch.arange(29)[:, None] == 3, float("inf"), v), f, None), (v.long(), f, None), (v, f, v[:5]), (v, f, v.long())):
        with pytest.raises(ValueError, match="repair_mesh"):
            MR.repair_mesh(bv, bf, bc, device="cpu")
    with pytest.raises(ValueError, match="weld_remap"):
        MR.weld_remap(nan, device="cpu")
    with pytest.raises(ValueError, match="drop_flags"):
        MR.drop_flags(v, f.float(), device="cpu")
    with pytest.raises(ValueError, match="orient_faces"):
        MR.orient_faces(v[:0], f, device="cpu")


# ---- the script -----------------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_repair_mesh_options_parse_and_are_checked_before_the_library_is_imported(monkeypatch):
    mod = _entry("repair_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "m.ply", "-o", "r.ply"]))
    assert a == {"mesh": "m.ply", "out": "r.ply", "grow": 1, "max_rounds": 8, "max_hole_edges": None, "no_orient": False, "no_weld": False, "json": None,
                 "strict": False}
    b = vars(ap.parse_args(["--mesh", "m.obj", "-o", "r.ply", "--grow", "2", "--max_rounds", "3", "--max_hole_edges", "40", "--no_orient", "--no_weld",
                            "--json", "r.json", "--strict"]))
    assert (b["grow"], b["max_rounds"], b["max_hole_edges"], b["no_orient"], b["no_weld"], b["json"], b["strict"]) == (2, 3, 40, True, True, "r.json", True)
    for missing in ([], ["--mesh", "m.ply"], ["-o", "r.ply"]):
        with pytest.raises(SystemExit):
            ap.parse_args(missing)
    monkeypatch.setitem(sys.modules, "render_mesh", None)
    base = ["--mesh", "does/not/exist.ply", "-o", "does/not/out.ply"]
    for bad in (["--json", "out.txt"], ["--grow", "-1"], ["--grow", "65"], ["--max_rounds", "-1"], ["--max_hole_edges", "2"], ["-o", "out.obj"],
                ["-o", "does/not/exist.ply"], ["-o", "does/not/../not/exist.ply"], ["--mesh", "does/not/exist.glb"]):
        with pytest.raises(SystemExit):
            mod.main(base + bad)
    with pytest.raises(ImportError):                       # good arguments do reach the import
        mod.main(base)
    r = {"watertight": False, "faces": 12, "boundary_edges": 3, "non_manifold_edges": 1, "self_intersections": 4, "components": 2}
    assert mod.line("before", "m.ply", r) == ("[repair] before m.ply: NOT watertight; 12 triangles, 3 open and 1 non-manifold edges, 4 intersecting "
                                              "pairs, 2 components")
