"""The mesh decimation of libv3d_recon.so (csrc_recon/meshdecim.hip, v3d_amd/recon/mesh_decimate.py, scripts/pub/decimate_mesh.py) without a
GPU: header, ctypes table and exports agree, bad arguments are refused before any launch, the host API refuses what does not fit and answers
empty meshes and targets that ask for nothing without a launch, the script's options are pinned, and the restatement
(tests/mesh_decimate_ref.py) is honest: its quadrics are the index_add formulation's, its cost is the summed squared area-weighted plane
distance, its loop leaves closed manifolds of the asked size that stay near the sphere, and the planted cases of the GPU tests sit far from
the thresholds that float32 could move."""
import importlib.util
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import mesh_decimate_ref as Dm
import mesh_render_ref as M
from conftest import record_parity
from v3d_amd.recon import mesh_decimate as MD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIM_ENTRIES = {"v3d_recon_mesh_vertex_quadrics", "v3d_recon_mesh_decim_propose", "v3d_recon_mesh_decim_min_round", "v3d_recon_mesh_decim_accept",
                 "v3d_recon_mesh_decim_cut", "v3d_recon_mesh_decim_apply"}


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


# ---- library --------------------------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert DECIM_ENTRIES <= declared and DECIM_ENTRIES <= set(geometry.SIGNATURES)
    for name in DECIM_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert "Mesh decimation" in hdr and os.path.exists(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshdecim.hip"))
    src = open(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshdecim.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("namespace {")[1].lower()
    assert int(re.search(r"#define V3D_RECON_MESH_MAX_VALENCE (\d+)", hdr).group(1)) == MD.MAX_VALENCE_LIMIT


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p, q = 0x1000, 0x2000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731
    big = (2 ** 31 - 1) // 3 + 1                                      # 3 F would pass INT32_MAX

    def calls(fn, order, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in order])

    def refuses(name, call, pointers, counts=(dict(F=0), dict(V=0), dict(F=-2), dict(V=-1), dict(F=big))):
        for k in pointers:
            assert call(**{k: None}) == -1 and name in err() and "null" in err(), (name, k)
        for kw in counts:
            assert call(**kw) == -1 and name in err() and "positive" in err(), (name, kw)

    vq = calls(lib.v3d_recon_mesh_vertex_quadrics, ("verts", "V", "faces", "F", "ranges", "corners", "Q", "stream"),
               verts=p, V=8, faces=p, F=4, ranges=p, corners=p, Q=p, stream=None)
    refuses("v3d_recon_mesh_vertex_quadrics", vq, ("verts", "faces", "ranges", "corners", "Q"))
    pr = calls(lib.v3d_recon_mesh_decim_propose, ("verts", "V", "faces", "F", "ranges", "corners", "Q", "cap", "keys", "targets", "stream"),
               verts=p, V=8, faces=p, F=4, ranges=p, corners=p, Q=p, cap=24, keys=p, targets=p, stream=None)
    refuses("v3d_recon_mesh_decim_propose", pr, ("verts", "faces", "ranges", "corners", "Q", "keys", "targets"))
    for cap in (2, 0, -1, MD.MAX_VALENCE_LIMIT + 1):
        assert pr(cap=cap) == -1 and "v3d_recon_mesh_decim_propose" in err() and "max_valence" in err(), cap
    mr = calls(lib.v3d_recon_mesh_decim_min_round, ("faces", "F", "ranges", "corners", "V", "kin", "kout", "stream"),
               faces=p, F=4, ranges=p, corners=p, V=8, kin=p, kout=q, stream=None)
    refuses("v3d_recon_mesh_decim_min_round", mr, ("faces", "ranges", "corners", "kin", "kout"))
    assert mr(kout=p) == -1 and "two buffers" in err()
    ac = calls(lib.v3d_recon_mesh_decim_accept, ("keys", "min2", "V", "max_error", "accept", "sel_keys", "sel_vals", "flags", "stream"),
               keys=p, min2=p, V=8, max_error=float("inf"), accept=p, sel_keys=p, sel_vals=p, flags=p, stream=None)
    refuses("v3d_recon_mesh_decim_accept", ac, ("keys", "min2", "accept", "sel_keys", "sel_vals", "flags"), counts=(dict(V=0), dict(V=-1)))
    for bad in (-1.0, float("nan"), float("-inf")):
        assert ac(max_error=bad) == -1 and "v3d_recon_mesh_decim_accept" in err() and "max_error" in err(), bad
    ct = calls(lib.v3d_recon_mesh_decim_cut, ("keys", "vals", "V", "live", "target", "accept", "stream"), keys=p, vals=p, V=8, live=p, target=4, accept=p,
               stream=None)
    refuses("v3d_recon_mesh_decim_cut", ct, ("keys", "vals", "live", "accept"), counts=(dict(V=0), dict(V=-1)))
    assert ct(target=-1) == -1 and "v3d_recon_mesh_decim_cut" in err() and "target_faces" in err()
    ap = calls(lib.v3d_recon_mesh_decim_apply, ("fin", "F", "V", "accept", "targets", "fout", "live", "Q", "removed", "stream"),
               fin=p, F=4, V=8, accept=p, targets=p, fout=q, live=p, Q=p, removed=p, stream=None)
    refuses("v3d_recon_mesh_decim_apply", ap, ("fin", "accept", "targets", "fout", "live", "Q", "removed"))
    assert ap(fout=p) == -1 and "two buffers" in err()


# ---- host API -------------------------------------------------------------------------------------------------------------------------------
def test_host_api_refuses_what_does_not_fit():
    v, f = M.icosphere(0)
    c = M.position_colors(v)
    V = v.shape[0]
    cpu = dict(device="cpu")
    Q = torch.zeros(V, 10, dtype=torch.float64)
    keys = torch.full((V,), -1, dtype=torch.int64)
    ints = torch.zeros(V, dtype=torch.int32)
    for call in (lambda ff: MD.decimate_mesh(v, ff, c, 4, **cpu), lambda ff: MD.vertex_quadrics(v, ff, **cpu), lambda ff: MD.propose(v, ff, Q, **cpu),
                 lambda ff: MD.select(ff, V, keys, **cpu), lambda ff: MD.apply(ff, V, ints, ints, Q, **cpu)):
        with pytest.raises(ValueError, match="outside the vertex array"):
            call(f + 1)
        with pytest.raises(ValueError, match="outside the vertex array"):
            call(f - 1)
        with pytest.raises(ValueError, match="must be integers"):
            call(f.float())
        with pytest.raises(ValueError, match=r"must be \[F, 3\]"):
            call(f.reshape(-1))
    with pytest.raises(ValueError, match=r"verts must be \[V, 3\]"):
        MD.decimate_mesh(v.reshape(-1), f, c, 4, **cpu)
    with pytest.raises(ValueError, match="verts must be floating point"):
        MD.decimate_mesh(v.long(), f, c, 4, **cpu)
    with pytest.raises(ValueError, match="12 vertices, 11 colours"):
        MD.decimate_mesh(v, f, c[:-1], 4, **cpu)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="target_faces"):
            MD.decimate_mesh(v, f, c, bad, **cpu)
    for kw in (dict(max_error=-1e-3), dict(max_error=float("nan")), dict(max_valence=2), dict(max_valence=MD.MAX_VALENCE_LIMIT + 1), dict(max_valence=6.5),
               dict(max_rounds=-1)):
        with pytest.raises(ValueError, match="max_error|max_valence|max_rounds"):
            MD.decimate_mesh(v, f, c, 4, **kw, **cpu)
    with pytest.raises(ValueError, match="max_valence"):
        MD.propose(v, f, Q, max_valence=1, **cpu)
    with pytest.raises(ValueError, match=r"quadrics must be float64 \[12, 10\]"):
        MD.propose(v, f, Q.float(), **cpu)
    with pytest.raises(ValueError, match=r"quadrics must be float64 \[12, 10\]"):
        MD.apply(f, V, ints, ints, Q[:-1], **cpu)
    with pytest.raises(ValueError, match=r"keys must be int64 \[12\]"):
        MD.select(f, V, keys[:-1], **cpu)
    with pytest.raises(ValueError, match=r"keys must be int64 \[12\]"):
        MD.select(f, V, keys.int(), **cpu)
    with pytest.raises(ValueError, match="max_error"):
        MD.select(f, V, keys, max_error=-1.0, **cpu)
    with pytest.raises(ValueError, match=r"accept must be integers \[12\]"):
        MD.apply(f, V, ints[:-1], ints, Q, **cpu)
    with pytest.raises(ValueError, match=r"targets must be integers \[12\]"):
        MD.apply(f, V, ints, ints.float(), Q, **cpu)
    with pytest.raises(ValueError, match="live_faces|target_faces"):
        MD.cut(keys, ints, -1, 4, **cpu)
    with pytest.raises(ValueError, match="live_faces|target_faces"):
        MD.cut(keys, ints, 20, -4, **cpu)
    with pytest.raises(ValueError, match=r"keys must be int64"):
        MD.cut(keys[:-1], ints, 20, 4, **cpu)


def test_nothing_to_do_is_answered_without_a_launch():
    cpu = dict(device="cpu")
    v, f = M.icosphere(0)
    c = M.position_colors(v)
    none = torch.zeros(0, 3, dtype=torch.int64)
    for vv, ff, cc, target in ((v, none, c, 0), (v[:0], none, c[:0], 5), (v, f, c, 20), (v, f, c, 21), (v, f, None, 10 ** 12)):
        ov, of, oc, st = MD.decimate_mesh(vv, ff, cc, target, **cpu)
        assert torch.equal(ov, vv) and torch.equal(of.long(), ff) and of.dtype == torch.int32 and (oc is None if cc is None else torch.equal(oc, cc))
        assert st["rounds"] == 0 and st["accepted"] == [] and st["reached"] and st["stopped"] == "target" and st["max_cost"] == 0.0
        assert st["faces_before"] == st["faces_after"] == ff.shape[0] and st["vertices_before"] == st["vertices_after"] == vv.shape[0]
        json.loads(json.dumps(st, allow_nan=False))
    for vv in (v, v[:0]):
        V = vv.shape[0]
        Q = MD.vertex_quadrics(vv, none, **cpu)
        assert Q.dtype == torch.float64 and tuple(Q.shape) == (V, 10) and not Q.any()
        keys, targets = MD.propose(vv, none, Q, **cpu)
        assert keys.dtype == torch.int64 and keys.tolist() == [-1] * V and targets.tolist() == [-1] * V
        accept, flags = MD.select(none, V, keys, **cpu)
        assert accept.tolist() == [0] * V and flags == (False, False)
        fo, live, Qo = MD.apply(none, V, accept, targets, Q, **cpu)
        assert fo.shape == (0, 3) and live.numel() == 0 and torch.equal(Qo, Q)
    assert MD.cut(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 10, 4, **cpu).numel() == 0
    assert torch.isnan(MD.cost_of_key(torch.tensor([-1]))).all() and MD.cost_of_key(torch.tensor([0x3F800000 << 32 | 7])).tolist() == [1.0]


# ---- the restatement against the textbook form ----------------------------------------------------------------------------------------------
def _planes(v, f):
    p = v.double()
    n = torch.linalg.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    ln = n.norm(dim=1, keepdim=True)
    unit = n / ln
    return unit, -(unit * p[f[:, 0]]).sum(1), 0.5 * ln[:, 0]


@pytest.mark.parametrize("name", ("ico2", "net", "noisy", "bipyramid", "grid", "unreferenced", "dart"))
def test_restatement_quadrics_are_the_index_add_formulation(name):
    v, f, _ = Dm.scene(name)
    V = v.shape[0]
    unit, d, w = _planes(v, f)
    plane = torch.cat([unit, d[:, None]], 1)
    outer = w[:, None, None] * plane[:, :, None] * plane[:, None, :]
    iu = torch.triu_indices(4, 4)
    want = torch.zeros(V, 10, dtype=torch.float64)
    for k in range(3):
        want.index_add_(0, f[:, k], outer[:, iu[0], iu[1]])
    mine = torch.from_numpy(Dm.vertex_quadrics(v, f))
    assert float((mine - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    mine32 = Dm.vertex_quadrics(v, f, np.float32)
    assert mine32.dtype == np.float32 and float(np.abs(mine32.astype(np.float64) - mine.numpy()).max()) < 1e-5 * max(1.0, float(want.abs().max()))
    if name == "unreferenced":
        used = torch.zeros(V, dtype=torch.bool)
        used[f.reshape(-1)] = True
        assert int((~used).sum()) == 5 and not mine[~used].any()


def test_restatement_cost_is_the_summed_squared_plane_distance():
    v, f, _ = Dm.scene("ico2")
    faces = Dm.face_list(f)
    Q = Dm.vertex_quadrics(v, faces)
    info = Dm.analyse(v, faces, Q)
    unit, d, w = _planes(v, f)
    p = v.double()
    worst, seen = 0.0, 0
    for vtx, cand in enumerate(info):
        assert cand is not None and len(cand) in (5, 6)                     # a closed icosphere: every vertex is removable
        for u, c in cand.items():
            at = (f == vtx).any(1).double() + (f == u).any(1).double()     # a face on both vertices counts twice, as in Q_v + Q_u
            dist = (unit * p[u]).sum(1) + d
            want = float((at * w * dist * dist).sum())
            worst, seen = max(worst, abs(c["cost"] - want)), seen + 1
            assert not c["why"] and all(x > 0 for x in c["dots"]) and len(c["dots"]) == len(cand) - 2
    print(f"{seen} collapses, cost against the plane-distance form: {worst:.3e}")
    assert seen == 2 * 480 and worst < 1e-15


# ---- the restatement's loop -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(Dm.LOOP_CASES))
def test_restatement_loop_leaves_a_closed_manifold_near_the_sphere(name):
    v, f, _ = Dm.scene(name)
    target = Dm.LOOP_CASES[name]
    kept, faces, st = Dm.decimate(v, f, target)
    rep = Dm.manifold_report(faces, kept.shape[0])
    meas = Dm.sphere_measures(v.numpy()[kept], faces, v, f)
    print(f"{name}: {f.shape[0]} -> {faces.shape[0]} faces in {st['rounds']} rounds, largest cost {st['max_cost']:.3e}; {rep}; {meas}")
    record_parity(f"mesh_decimate_restatement[{name}]", {"faces_before": int(f.shape[0]), "faces_after": int(faces.shape[0]), "rounds": st["rounds"],
                                                         "max_cost": st["max_cost"], **meas})
    assert Dm.manifold_report(f, v.shape[0])["edges_twice_opposite"] and Dm.manifold_report(f, v.shape[0])["euler"] == 2
    assert rep == {"edges_twice_opposite": True, "euler": 2, "duplicates": 0, "degenerate": 0, "used_vertices": kept.shape[0]}
    assert faces.shape[0] in (target, target - 1) and st["reached"] and sum(st["accepted"]) * 2 == f.shape[0] - faces.shape[0]
    assert np.all(np.diff(kept) > 0) and kept.shape[0] == v.shape[0] - sum(st["accepted"])           # a subset of the input, in its order
    # a coarser polyhedron inscribed in the same sphere: its faces dip below it by about edge^2 / (8 r), and it loses volume, not shape
    assert meas["radial"] < 0.05 and 0.9 < meas["volume_ratio"] <= 1.0


def test_restatement_loop_may_skip_the_vertices_nothing_touched():
    v, f, _ = Dm.scene("ico2")
    a, b = Dm.decimate(v, f, 61), Dm.decimate(v, f, 61, incremental=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[1].shape[0] == 60          # 320 - 61 is odd: one less


def test_planted_cases_sit_far_from_their_thresholds():
    """What decides validity in the scenes of the GPU tests, on the restatement alone"""
    # no scene of the validity tests has a flip decision that float32 could take the other way; the noisy sphere has flips, all of them clear
    for name in ("tetrahedron", "octahedron", "grid", "flat", "bipyramid", "dart", "unreferenced", "ico2", "ico3", "net", "noisy"):
        v, f, _ = Dm.scene(name)
        faces = Dm.face_list(f)
        i64 = Dm.analyse(v, faces, Dm.vertex_quadrics(v, faces))
        i32 = Dm.analyse(v, faces, Dm.vertex_quadrics(v, faces, np.float32), dtype=np.float32)
        assert all(Dm.clear_of_the_flip_threshold(i64, i32)), name
        flips = sum("flip" in c["why"] for cand in i64 if cand for c in cand.values())
        assert (flips > 100) if name == "noisy" else (flips == (2 if name == "dart" else flips)), (name, flips)
        assert [[u for u, c in cand.items() if not c["why"]] if cand else None for cand in i64] == \
               [[u for u, c in cand.items() if not c["why"]] if cand else None for cand in i32], name
    # the tetrahedron: every collapse would repeat the face opposite; the octahedron: every collapse is valid
    for name, want in (("tetrahedron", {"duplicate"}), ("octahedron", set())):
        v, f, _ = Dm.scene(name)
        info = Dm.analyse(v, Dm.face_list(f), Dm.vertex_quadrics(v, f))
        assert all(c["why"] == want for cand in info for c in cand.values()) and all(len(cand) == (3 if name == "tetrahedron" else 4) for cand in info)
    # the dart: the tips flip a face, far from 0 in both precisions
    v, f, _ = Dm.scene("dart")
    faces = Dm.face_list(f)
    i64 = Dm.analyse(v, faces, Dm.vertex_quadrics(v, faces))
    i32 = Dm.analyse(v, faces, Dm.vertex_quadrics(v, faces, np.float32), dtype=np.float32)
    assert [x is not None for x in i64] == [True, False, False, False, False]
    d = Dm.DART
    for tip in (d["left"], d["right"]):
        assert i64[0][tip]["why"] == {"flip"} == i32[0][tip]["why"] and min(i64[0][tip]["dots"]) < -0.4
    for ok in (d["top"], d["notch"]):
        assert not i64[0][ok]["why"] and min(i64[0][ok]["dots"]) > 0.3
    for u in i64[0]:
        assert max(abs(float(a) - b) for a, b in zip(i32[0][u]["dots"], i64[0][u]["dots"])) < 1e-6
    # the open grid: the rim is open, the interior is not; the flat one costs exactly nothing anywhere
    for name in ("grid", "flat"):
        v, f, _ = Dm.scene(name)
        info = Dm.analyse(v, Dm.face_list(f), Dm.vertex_quadrics(v, f))
        assert [x is not None for x in info] == (~Dm.grid_rim()).tolist() and v.shape[0] > 256
        if name == "flat":
            assert all(c["cost"] == 0.0 for cand in info if cand for c in cand.values())
    # the two fans on one rim: the apexes are over the cap; a rim vertex may go to either rim neighbour and to neither apex
    v, f, _ = Dm.scene("bipyramid")
    info = Dm.analyse(v, Dm.face_list(f), Dm.vertex_quadrics(v, f))
    assert f.shape[0] == Dm.FAN and info[0] is None and info[1] is None
    for vtx in range(2, v.shape[0]):
        assert all("valence" in info[vtx][apex]["why"] for apex in (0, 1))
        assert all(not c["why"] for u, c in info[vtx].items() if u >= 2) and len(info[vtx]) == 4
    lifted = Dm.analyse(v, Dm.face_list(f), Dm.vertex_quadrics(v, f), max_valence=1024, only=(0, 1))
    assert lifted[0] is not None and len(lifted[1]) == Dm.FAN // 2                       # it is the cap alone that keeps the apexes
    # the cap on the target alone: on the 320-face icosphere (12 vertices of 5 faces, never adjacent, the others of 6) a collapse leaves its
    # target with 7 or 8 faces: none is valid under a cap of 6, those between a 5 and a 6 under a cap of 7, all under 8
    v, f, _ = Dm.scene("ico2")
    faces = Dm.face_list(f)
    size = [len(s) for s in Dm.stars(faces, v.shape[0])]
    for cap, want in ((6, set()), (7, {(5, 6), (6, 5)}), (8, {(5, 6), (6, 5), (6, 6)})):
        info = Dm.analyse(v, faces, Dm.vertex_quadrics(v, faces), max_valence=cap)
        assert all(c["why"] <= {"valence"} for cand in info for c in cand.values())
        assert {(size[vtx], size[u]) for vtx, cand in enumerate(info) for u, c in cand.items() if not c["why"]} == want, cap


# ---- script and files -----------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_are_pinned():
    mod = _entry("decimate_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh.ply", "-o", "out/gs/mesh_50k.ply"]))
    assert a == {"mesh": "out/gs/mesh.ply", "out": "out/gs/mesh_50k.ply", "target_faces": 50000, "max_error": None, "max_valence": 24,
                 "white_background": False, "render_orbit": 0, "video": None, "num_frames": None, "reso": None, "radius": 2.0, "elevation": 0.0,
                 "fov": 60.0}
    b = vars(ap.parse_args(["--mesh", "in.ply", "-o", "out.ply", "--target_faces", "50000", "--max_error", "1e-6", "--render_orbit", "36", "-w", "--video",
                            "orbit.npy", "--max_valence", "16", "--num_frames", "18", "--reso", "64", "--radius", "3", "--elevation", "10", "--fov", "45"]))
    assert b == {"mesh": "in.ply", "out": "out.ply", "target_faces": 50000, "max_error": 1e-6, "max_valence": 16, "white_background": True,
                 "render_orbit": 36, "video": "orbit.npy", "num_frames": 18, "reso": 64, "radius": 3.0, "elevation": 10.0, "fov": 45.0}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov", "white_background"):
        assert a[k] == recon[k], k
    with pytest.raises(SystemExit):
        ap.parse_args(["-o", "c.ply"])                   # --mesh is required
    with pytest.raises(SystemExit):
        ap.parse_args(["--mesh", "m.ply"])               # -o is required
    for bad in (["--target_faces", "-1"], ["--max_error", "-1"], ["--max_error", "nan"], ["--max_valence", "2"], ["--render_orbit", "-1"], ["--reso", "0"],
                ["--reso", "5000"]):
        with pytest.raises(SystemExit):
            mod.main(["--mesh", "does/not/exist.ply", "-o", "c.ply", *bad])
    lib_defaults = {k: p.default for k, p in inspect.signature(MD.decimate_mesh).parameters.items()}          # the script's defaults are the library's
    assert a["max_error"] == lib_defaults["max_error"] and a["max_valence"] == lib_defaults["max_valence"] == MD.DEFAULT_MAX_VALENCE == Dm.DEFAULT_MAX_VALENCE
    assert "decimate_mesh.py" in open(os.path.join(ROOT, "README.md")).read()


def test_script_writes_strict_json_and_a_ply_that_loads(tmp_path):
    """Without a GPU only a mesh that needs nothing gets through (no launch): the files are written all the same."""
    from v3d_amd.recon import geometry as G
    v, f = M.icosphere(0)
    ply, out = str(tmp_path / "mesh.ply"), str(tmp_path / "small.ply")
    G.save_mesh_ply(ply, v, f, M.position_colors(v))
    _entry("decimate_mesh").main(["--mesh", ply, "-o", out, "--target_faces", "20"], device="cpu")
    assert sorted(os.listdir(tmp_path)) == ["mesh.ply", "small.json", "small.ply"]

    def strict(token):
        raise ValueError(f"{token} is not JSON")
    stats = json.loads(open(tmp_path / "small.json").read(), parse_constant=strict)
    assert stats["faces_before"] == 20 == stats["faces_after"] and stats["reached"] and stats["rounds"] == 0 and stats["vertices_after"] == 12
    assert {"rounds", "accepted", "faces_before", "faces_after", "reached", "max_cost", "boundary_vertices_before", "boundary_vertices_after"} <= set(stats)
    rv, rf, rc = G.read_mesh_ply(out)
    rv0, rf0, rc0 = G.read_mesh_ply(ply)
    assert np.array_equal(rv, rv0) and np.array_equal(rf, rf0) and np.array_equal(rc, rc0)
