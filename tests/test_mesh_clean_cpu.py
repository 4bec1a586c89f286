"""The mesh cleaning of libv3d_recon.so (csrc_recon/meshtopo.hip, v3d_amd/recon/mesh_clean.py, scripts/pub/clean_mesh.py) without a GPU:
header, ctypes table and exports agree, bad arguments are refused before any launch, the host API refuses what does not fit and answers
empty meshes without a launch, the script's options are pinned, and the torch restatement (tests/mesh_clean_ref.py) is honest: its
components are a union-find's, its normals are the index_add formulation's, its Taubin smoothing smooths without shrinking, and every test
scene keeps its normal sums clear of the degenerate-normal threshold."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_clean_ref as C
import mesh_render_ref as M
import recon_geom_ref as R
from v3d_amd.recon import mesh_clean as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPO_ENTRIES = {"v3d_recon_mesh_corner_records", "v3d_recon_mesh_vertex_normals", "v3d_recon_mesh_label_round", "v3d_recon_mesh_face_labels",
                "v3d_recon_mesh_keep_flags", "v3d_recon_mesh_compact_faces", "v3d_recon_mesh_boundary_flags", "v3d_recon_mesh_smooth_pass"}


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
    assert TOPO_ENTRIES <= declared and TOPO_ENTRIES <= set(geometry.SIGNATURES)
    for name in TOPO_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert "Mesh topology" in hdr and os.path.exists(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshtopo.hip"))


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p, q = 0x1000, 0x2000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731
    big = (2 ** 31 - 1) // 3 + 1                                      # 3 F would pass INT32_MAX

    def calls(fn, order, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in order])

    def refuses(name, call, pointers):
        for k in pointers:
            assert call(**{k: None}) == -1 and name in err() and "null" in err(), (name, k)
        for kw in (dict(F=0), dict(V=0), dict(F=-2), dict(V=-1), dict(F=big)):
            assert call(**kw) == -1 and name in err() and "positive" in err(), (name, kw)

    cr = calls(lib.v3d_recon_mesh_corner_records, ("faces", "F", "V", "keys", "vals", "stream"), faces=p, F=4, V=8, keys=p, vals=p, stream=None)
    refuses("v3d_recon_mesh_corner_records", cr, ("faces", "keys", "vals"))
    vn = calls(lib.v3d_recon_mesh_vertex_normals, ("verts", "V", "faces", "F", "ranges", "corners", "normals", "stream"),
               verts=p, V=8, faces=p, F=4, ranges=p, corners=p, normals=p, stream=None)
    refuses("v3d_recon_mesh_vertex_normals", vn, ("verts", "faces", "ranges", "corners", "normals"))
    lr = calls(lib.v3d_recon_mesh_label_round, ("faces", "F", "ranges", "corners", "V", "lin", "lout", "changed", "stream"),
               faces=p, F=4, ranges=p, corners=p, V=8, lin=p, lout=q, changed=p, stream=None)
    refuses("v3d_recon_mesh_label_round", lr, ("faces", "ranges", "corners", "lin", "lout", "changed"))
    assert lr(lout=p) == -1 and "two buffers" in err()
    fl = calls(lib.v3d_recon_mesh_face_labels, ("faces", "F", "labels", "V", "keys", "vals", "stream"), faces=p, F=4, labels=p, V=8, keys=p, vals=p,
               stream=None)
    refuses("v3d_recon_mesh_face_labels", fl, ("faces", "labels", "keys", "vals"))
    kf = calls(lib.v3d_recon_mesh_keep_flags, ("faces", "F", "ranges", "corners", "V", "labels", "keep_root", "keep_face", "keep_vert", "stream"),
               faces=p, F=4, ranges=p, corners=p, V=8, labels=p, keep_root=p, keep_face=p, keep_vert=p, stream=None)
    refuses("v3d_recon_mesh_keep_flags", kf, ("faces", "ranges", "corners", "labels", "keep_root", "keep_face", "keep_vert"))
    cf = calls(lib.v3d_recon_mesh_compact_faces, ("faces", "F", "V", "keep_face", "face_off", "keep_vert", "vert_off", "Fo", "Vo", "out", "stream"),
               faces=p, F=4, V=8, keep_face=p, face_off=p, keep_vert=p, vert_off=p, Fo=2, Vo=4, out=p, stream=None)
    refuses("v3d_recon_mesh_compact_faces", cf, ("faces", "keep_face", "face_off", "keep_vert", "vert_off", "out"))
    for kw in (dict(Fo=0), dict(Fo=5), dict(Vo=0), dict(Vo=9)):
        assert cf(**kw) == -1 and "v3d_recon_mesh_compact_faces" in err() and "out of 4 and 8" in err(), kw
    bf = calls(lib.v3d_recon_mesh_boundary_flags, ("faces", "F", "ranges", "corners", "V", "flags", "stream"), faces=p, F=4, ranges=p, corners=p, V=8,
               flags=p, stream=None)
    refuses("v3d_recon_mesh_boundary_flags", bf, ("faces", "ranges", "corners", "flags"))
    sp = calls(lib.v3d_recon_mesh_smooth_pass, ("vin", "V", "faces", "F", "ranges", "corners", "pinned", "factor", "vout", "stream"),
               vin=p, V=8, faces=p, F=4, ranges=p, corners=p, pinned=None, factor=0.5, vout=q, stream=None)
    refuses("v3d_recon_mesh_smooth_pass", sp, ("vin", "faces", "ranges", "corners", "vout"))            # (pinned may be null)
    assert sp(vout=p) == -1 and "two buffers" in err()
    assert sp(factor=float("nan")) == -1 and "finite" in err()
    assert sp(factor=float("inf")) == -1 and "finite" in err()


# ---- host API -------------------------------------------------------------------------------------------------------------------------------
def test_host_api_refuses_what_does_not_fit():
    v, f = M.icosphere(0)
    c = M.position_colors(v)
    V = v.shape[0]
    cpu = dict(device="cpu")
    for call in (lambda ff: MC.vertex_corners(ff, V, **cpu), lambda ff: MC.vertex_components(ff, V, **cpu), lambda ff: MC.boundary_vertices(ff, V, **cpu),
                 lambda ff: MC.vertex_normals(v, ff, **cpu), lambda ff: MC.taubin_smooth(v, ff, **cpu), lambda ff: MC.filter_components(v, ff, c, **cpu),
                 lambda ff: MC.clean_mesh(v, ff, c, **cpu), lambda ff: MC.render_mesh_normals(D.cams_for(32, 32)[0], v, ff, **cpu)):
        with pytest.raises(ValueError, match="outside the vertex array"):
            call(f + 1)
        with pytest.raises(ValueError, match="outside the vertex array"):
            call(f - 1)
        with pytest.raises(ValueError, match="must be integers"):
            call(f.float())
        with pytest.raises(ValueError, match=r"must be \[F, 3\]"):
            call(f.reshape(-1))
    with pytest.raises(ValueError, match="num_verts"):
        MC.vertex_corners(f[:0], -1, **cpu)
    with pytest.raises(ValueError, match=r"verts must be \[V, 3\]"):
        MC.vertex_normals(v.reshape(-1), f, **cpu)
    with pytest.raises(ValueError, match="verts must be floating point"):
        MC.taubin_smooth(v.long(), f, **cpu)
    with pytest.raises(ValueError, match="12 vertices, 11 colours"):
        MC.filter_components(v, f, c[:-1], **cpu)
    with pytest.raises(ValueError, match="12 vertices, 11 colours"):
        MC.render_mesh_normals(D.cams_for(32, 32)[0], v, f, normals=c[:-1], **cpu)
    for kw in (dict(min_faces=-1), dict(keep_largest=-1), dict(min_faces=1.5)):
        with pytest.raises(ValueError, match="must be an integer that is not negative"):
            MC.filter_components(v, f, c, **kw, **cpu)
        with pytest.raises(ValueError, match="must be an integer that is not negative"):
            MC.clean_mesh(v, f, c, **kw, **cpu)
    for kw in (dict(iterations=-1), dict(lam=float("nan")), dict(mu=float("inf"))):
        with pytest.raises(ValueError, match="iterations|finite"):
            MC.taubin_smooth(v, f, **kw, **cpu)
        with pytest.raises(ValueError, match="iterations|finite"):
            MC.clean_mesh(v, f, c, **kw, **cpu)


def test_empty_meshes_are_answered_without_a_launch():
    cpu = dict(device="cpu")
    v, _ = M.icosphere(0)
    c = M.position_colors(v)
    none = torch.zeros(0, 3, dtype=torch.int64)
    for vv, cc in ((v, c), (v[:0], c[:0])):
        V = vv.shape[0]
        ranges, corners = MC.vertex_corners(none, V, **cpu)
        assert tuple(ranges.shape) == (V, 2) and ranges.dtype == torch.int32 and not ranges.any() and corners.numel() == 0
        labels, rounds = MC.vertex_components(none, V, **cpu)
        assert labels.tolist() == list(range(V)) and rounds == 0
        assert torch.equal(MC.vertex_normals(vv, none, **cpu), torch.tensor([[0.0, 0.0, 1.0]]).expand(V, 3))
        assert not MC.boundary_vertices(none, V, **cpu).any() and MC.boundary_vertices(none, V, **cpu).shape[0] == V
        assert torch.equal(MC.taubin_smooth(vv, none, **cpu), vv)
        fv, ff, fc, st = MC.filter_components(vv, none, cc, **cpu)
        assert fv.shape == (0, 3) and ff.shape == (0, 3) and fc.shape == (0, 3) and ff.dtype == torch.int32
        assert st["removed_vertices"] == V == st["unreferenced_vertices"] and st["components_before"] == [] == st["components_after"]
        cv, cf, ccol, cs = MC.clean_mesh(vv, none, cc, **cpu)
        assert cv.shape == (0, 3) and cf.shape == (0, 3) and cs["vertices"] == 0 == cs["faces"] and cs["removed_vertices"] == V
        cv, cf, ccol, cs = MC.clean_mesh(vv, none, cc, min_faces=0, **cpu)             # the filter left out: the loose vertices stay
        assert torch.equal(cv, vv) and torch.equal(ccol, cc) and cs["removed_vertices"] == 0 and not cs["filtered"]
        json.loads(json.dumps(cs, allow_nan=False))
        out = MC.render_mesh_normals(D.cams_for(40, 24)[1], vv, none, bg=(0.25, 0.5, 1.0), **cpu)
        assert torch.equal(out["render"][:, 3, 5], torch.tensor([0.25, 0.5, 1.0])) and not out["alpha"].any()
    frames = MC.render_normal_orbit(v, none, 3, 2.0, 0.0, 60.0, 16, **cpu)
    assert frames.shape == (3, 16, 16, 3) and frames.dtype == np.uint8 and bool((frames == 255).all())
    # taubin with no iteration returns the vertices, without a launch
    _, f = M.icosphere(0)
    assert torch.equal(MC.taubin_smooth(v, f, iterations=0, **cpu), v)


def test_keep_rule_and_normal_colours():
    table = [{"root": 0, "faces": 320, "vertices": 162}, {"root": 3, "faces": 1, "vertices": 3}, {"root": 9, "faces": 320, "vertices": 162},
             {"root": 20, "faces": 4, "vertices": 4}, {"root": 40, "faces": 500, "vertices": 300}]
    for mf, kl in ((0, 0), (2, 0), (64, 0), (8, 1), (0, 2), (0, 3), (321, 2), (501, 0), (4, 9)):
        assert MC.kept_roots(table, mf, kl) == C.kept_roots(list(table), mf, kl), (mf, kl)
    assert MC.kept_roots(table, 64, 0) == [0, 9, 40] and MC.kept_roots(table, 0, 2) == [0, 40] and MC.kept_roots(table, 0, 1) == [40]
    assert MC.kept_roots(table[:4], 0, 1) == [0]                      # equal sizes: the smaller root
    assert MC.kept_roots(table, 501, 0) == []
    # normals as colours: x right, y up, z towards the camera
    cam = D.cams_for(32, 32)[0]
    eye = cam.center / cam.center.norm()
    Rm = cam.world_view[:3, :3]
    right, down = Rm[:, 0], Rm[:, 1]
    col = MC.normal_colors(cam, torch.stack([eye, right, -down, -eye]))
    want = torch.tensor([[0.5, 0.5, 1.0], [1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 0.0]])
    assert float((col - want).abs().max()) < 1e-6


# ---- the restatement's own honesty ------------------------------------------------------------------------------------------------------------
def union_find(faces, V):
    """labels [V]: the smallest index of every vertex's component"""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in faces.tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return torch.tensor([find(x) for x in range(V)])


def scenes():
    """name -> (verts, faces, colors): every mesh the GPU tests feed the kernels"""
    out = {"sphere": M.mesh_scene("sphere", M.SEEDS["sphere"]), "pair": M.mesh_scene("pair", M.SEEDS["pair"]), "fan": C.fan(), "triangle": C.triangle(),
           "unreferenced": C.insert_unreferenced(*M.mesh_scene("sphere", M.SEEDS["sphere"]))[:3],
           "degenerate": C.add_degenerate(*M.mesh_scene("sphere", M.SEEDS["sphere"])), "floaters": C.floater_scene()[:3],
           "strip": C.quad_strip(500, seed=4)[:3], "net": C.sphere_mesh(), "noisy": C.noisy_sphere(0), "grid": C.open_grid()}
    return out


def test_restatement_components_are_union_find():
    for name, (v, f, c) in scenes().items():
        V = v.shape[0]
        labels, rounds = C.components(f, V)
        slow, slow_rounds = C.components(f, V, jump=False)
        assert torch.equal(labels, union_find(f, V)) and torch.equal(slow, labels), name
        assert 1 <= rounds <= slow_rounds <= V + 8, name
        print(f"{name}: {V} vertices, {len(C.component_table(f, V, labels))} components with faces, rounds {rounds} (without the jump {slow_rounds})")
    v, f, c, perm = C.floater_scene()
    labels, _ = C.components(f, v.shape[0])
    table = C.component_table(f, v.shape[0], labels)
    assert sorted(r["faces"] for r in table) == [1, 1, 4, 320, 320] and sorted(r["vertices"] for r in table) == [3, 3, 4, 162, 162]
    assert v.shape[0] - sum(r["vertices"] for r in table) == 3
    # the figures of the write-up: the sphere nets in raster vertex order, a strip in natural and in permuted order
    assert [C.components(C.sphere_mesh(N)[1], C.sphere_mesh(N)[0].shape[0])[1] for N in (24, 48)] == [6, 7]
    assert C.components(C.quad_strip(500)[1], 1002)[1] < 20 < 100 < C.components(C.quad_strip(500, seed=4)[1], 1002)[1] <= 1002 + 8


def test_restatement_lists_and_normals():
    for name, (v, f, c) in scenes().items():
        V = v.shape[0]
        ranges, corners = C.corner_lists(f, V)
        flat = f.reshape(-1)
        for vtx in range(0, V, max(1, V // 50)):
            mine = corners[ranges[vtx, 0]:ranges[vtx, 1]].tolist()
            assert mine == torch.nonzero(flat == vtx).reshape(-1).tolist(), (name, vtx)          # its corners, ascending
        # the index_add formulation of the same normals
        p = v.double()
        fn = torch.linalg.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
        s = torch.zeros(V, 3, dtype=torch.float64)
        for k in range(3):
            s.index_add_(0, f[:, k], fn)
        mine = C.normal_sums(v, f)
        assert float((mine - s).abs().max()) <= 1e-12 * max(1.0, float(s.abs().max())), name
        # the degenerate-normal margin: exactly 0 or well above the threshold, so fp32 and fp64 take the same branch
        len2 = (mine * mine).sum(1)
        assert bool(((len2 == 0) | (len2 > C.NORMAL_MARGIN)).all()), (name, float(len2[len2 > 0].min()))
        n64, n32 = C.normals(v, f), C.normals(v, f, torch.float32)
        assert torch.equal(C.has_normal(v, f), C.has_normal(v, f, torch.float32)) and torch.equal(C.has_normal(v, f), len2 > 0), name
        assert float((n32.double() - n64).abs().max()) < 1e-5, name
        assert float((n64.norm(dim=1) - 1).abs().max()) < 1e-12
    v, f, c = scenes()["degenerate"]
    assert bool((C.normal_sums(v, f)[-6:] == 0).all()) and bool((C.normals(v, f)[-6:] == torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).all())
    v, f, c = C.sphere_mesh()
    cosine = (C.normals(v, f) * (v.double() / v.double().norm(dim=1, keepdim=True))).sum(1)
    print(f"sphere net: smallest n . v / |v| {float(cosine.min()):.4f}")
    assert float(cosine.min()) >= 0.99


def test_restatement_boundary():
    v, f, c = C.open_grid()
    flags = C.boundary_flags(f, v.shape[0])
    q, _, _ = M.quad_grid(split=2)
    rim = (q[:, 0] == q[:, 0].min()) | (q[:, 0] == q[:, 0].max()) | (q[:, 1] == q[:, 1].min()) | (q[:, 1] == q[:, 1].max())
    assert torch.equal(flags.bool(), rim) and 0 < int(flags.sum()) < v.shape[0]
    for name in ("sphere", "net", "fan"):
        vv, ff, _ = scenes()[name]
        want = 0 if name != "fan" else C.FAN                          # the fan's ring is open, its centre is not
        assert int(C.boundary_flags(ff, vv.shape[0]).sum()) == want, name
    und, cnt, _ = R.undirected_counts(C.sphere_mesh()[1])
    assert bool((cnt == 2).all())


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_restatement_taubin_smooths_without_shrinking(seed):
    v, f, c = C.noisy_sphere(seed)
    rough0, vol0 = float(v.double().norm(dim=1).std()), R.signed_volume(v, f)
    out = C.taubin(v, f, 10, 0.5, -0.53)
    shrunk = C.taubin(v, f, 10, 0.5, 0.0)
    rough, vol, vol_mu0 = float(out.norm(dim=1).std()), R.signed_volume(out, f), R.signed_volume(shrunk, f)
    print(f"seed {seed}: std |v| {rough0:.4e} -> {rough:.4e} ({rough / rough0:.3f}); volume {vol / vol0 - 1:+.2%}; with mu = 0 {vol_mu0 / vol0 - 1:+.2%}")
    assert rough < 0.5 * rough0
    assert abs(vol / vol0 - 1) < 0.02
    assert vol_mu0 / vol0 - 1 < -0.10                                # the second pass is what keeps the volume
    pinned = C.taubin(*C.open_grid()[:2], 3, fix_boundary=True)
    flags = C.boundary_flags(C.open_grid()[1], pinned.shape[0]).bool()
    assert torch.equal(pinned[flags], C.open_grid()[0].double()[flags]) and not torch.equal(pinned[~flags], C.open_grid()[0].double()[~flags])


def test_restatement_filter_keeps_order():
    v, f, c, perm = C.floater_scene()
    fv, ff, fc, keep_face, keep_vert, table = C.filter_components(v, f, c, min_faces=8)
    assert fv.shape[0] == 2 * 162 and ff.shape[0] == 640 and int(keep_vert.sum()) == 324
    assert torch.equal(fv[ff], v[f[keep_face]])                        # the same triangles, in their order
    same = C.filter_components(*C.sphere_mesh(), min_faces=64)
    assert torch.equal(same[0], C.sphere_mesh()[0]) and torch.equal(same[1], C.sphere_mesh()[1])


# ---- script and files -----------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_are_pinned():
    ap = _entry("clean_mesh").build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh.ply", "-o", "out/gs/mesh_clean.ply"]))
    assert a == {"mesh": "out/gs/mesh.ply", "out": "out/gs/mesh_clean.ply", "white_background": False, "min_faces": 64, "keep_largest": 0, "smooth": 10,
                 "lam": 0.5, "mu": -0.53, "fix_boundary": False, "render_normals": 0, "reso": 512, "radius": 2.0, "elevation": 0.0, "fov": 60.0}
    b = vars(ap.parse_args(["--mesh", "m.ply", "-o", "c.ply", "--min_faces", "8", "--smooth", "0", "--render_normals", "36", "-w", "--keep_largest", "1",
                            "--lam", "0.4", "--mu", "-0.42", "--fix_boundary", "--reso", "64", "--radius", "3", "--elevation", "10", "--fov", "45"]))
    assert b == {"mesh": "m.ply", "out": "c.ply", "white_background": True, "min_faces": 8, "keep_largest": 1, "smooth": 0, "lam": 0.4, "mu": -0.42,
                 "fix_boundary": True, "render_normals": 36, "reso": 64, "radius": 3.0, "elevation": 10.0, "fov": 45.0}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov", "white_background"):
        assert a[k] == recon[k], k
    with pytest.raises(SystemExit):
        ap.parse_args(["-o", "c.ply"])                   # --mesh is required
    with pytest.raises(SystemExit):
        ap.parse_args(["--mesh", "m.ply"])               # -o is required
    mod = _entry("clean_mesh")
    for bad in (["--min_faces", "-1"], ["--smooth", "-2"], ["--keep_largest", "-1"], ["--lam", "nan"], ["--reso", "0"], ["--reso", "5000"]):
        with pytest.raises(SystemExit):
            mod.main(["--mesh", "does/not/exist.ply", "-o", "c.ply", *bad])
    import inspect
    lib_defaults = {k: p.default for k, p in inspect.signature(MC.clean_mesh).parameters.items()}          # the script's defaults are the library's
    for opt, arg in (("min_faces", "min_faces"), ("keep_largest", "keep_largest"), ("smooth", "iterations"), ("lam", "lam"), ("mu", "mu"),
                     ("fix_boundary", "fix_boundary")):
        assert a[opt] == lib_defaults[arg], opt


def test_script_writes_strict_json_and_a_ply_that_loads(tmp_path):
    """Without a GPU only a mesh without faces gets through (no launch): its loose vertices go, the files are written all the same."""
    from v3d_amd.recon import geometry as G
    v, _ = M.icosphere(0)
    ply, out = str(tmp_path / "mesh.ply"), str(tmp_path / "clean.ply")
    G.save_mesh_ply(ply, v, torch.zeros(0, 3, dtype=torch.int64), M.position_colors(v))
    _entry("clean_mesh").main(["--mesh", ply, "-o", out, "--render_normals", "2", "--reso", "16", "-w"], device="cpu")
    assert sorted(os.listdir(tmp_path)) == ["clean.json", "clean.ply", "clean_normals", "mesh.ply"]
    assert sorted(os.listdir(tmp_path / "clean_normals")) == ["000.png", "001.png", "orbit.npy"]

    def strict(token):
        raise ValueError(f"{token} is not JSON")
    stats = json.loads(open(tmp_path / "clean.json").read(), parse_constant=strict)
    assert stats["vertices_before"] == 12 and stats["vertices"] == 0 == stats["faces"] and stats["removed_vertices"] == 12 == stats["unreferenced_vertices"]
    assert {"components_before", "components_after", "removed_faces", "removed_vertices", "unreferenced_vertices", "boundary_vertices_before",
            "boundary_vertices_after", "rounds"} <= set(stats)
    rv, rf, rc = G.read_mesh_ply(out)
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rc.shape == (0, 3)
    assert np.load(tmp_path / "clean_normals" / "orbit.npy").shape == (2, 16, 16, 3)
