"""The mesh BVH and the normal bake of libv3d_recon.so (csrc_recon/meshbvh.hip, v3d_amd/recon/mesh_bake.py, scripts/pub/bake_normals.py)
without a GPU: header, ctypes table and exports agree, bad arguments are refused before any launch, the torch restatement
(tests/mesh_bake_ref.py) is honest (radial normals on an analytic sphere, a tree checker that accepts a right tree and refuses wrong ones),
the OBJ writer with and without a normal map, the script's options, and the premises of the cases of tests/test_mesh_bake_gpu.py on the
restatement alone."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import mesh_bake_ref as B
import mesh_clean_ref as C
import mesh_render_ref as M
import mesh_texture_ref as TX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BVH_ENTRIES = {"v3d_recon_bvh_face_keys", "v3d_recon_bvh_build_nodes", "v3d_recon_bvh_fit_round", "v3d_recon_bvh_closest_hit",
               "v3d_recon_tex_bake_normals"}
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


def test_header_signatures_and_exports_agree(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert BVH_ENTRIES <= declared and declared == set(geometry.SIGNATURES)
    for name in BVH_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert "Mesh BVH and normal bake" in hdr and "THE NODES" in hdr and re.search(r"#define V3D_RECON_BVH_STACK 64\b", hdr)
    src = open(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshbvh.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p, q = 0x1000, 0x2000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731

    def calls(fn, names, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in names])

    big = 2 ** 30 + 1
    fk = calls(lib.v3d_recon_bvh_face_keys, ("verts", "V", "faces", "F", "lx", "ly", "lz", "hx", "hy", "hz", "keys", "vals", "flo", "fhi", "stream"),
               verts=p, V=162, faces=p, F=320, lx=0.0, ly=0.0, lz=0.0, hx=1.0, hy=1.0, hz=1.0, keys=p, vals=p, flo=p, fhi=p, stream=None)
    for k in ("verts", "faces", "keys", "vals", "flo", "fhi"):
        assert fk(**{k: None}) == -1 and "v3d_recon_bvh_face_keys" in err() and "null" in err(), k
    assert fk(V=0) == -1 and "num_verts" in err()
    assert fk(F=0) == -1 and "num_faces 0" in err()
    assert fk(F=big) == -1 and "num_faces" in err()
    assert fk(hx=-1.0) == -1 and "bounding box" in err()
    assert fk(ly=float("nan")) == -1 and "bounding box" in err()
    assert fk(hz=float("inf")) == -1 and "bounding box" in err()
    bn = calls(lib.v3d_recon_bvh_build_nodes, ("keys", "order", "flo", "fhi", "F", "left", "right", "parent", "lo", "hi", "stream"),
               keys=p, order=p, flo=p, fhi=p, F=320, left=p, right=p, parent=p, lo=p, hi=p, stream=None)
    for k in ("keys", "order", "flo", "fhi", "left", "right", "parent", "lo", "hi"):
        assert bn(**{k: None}) == -1 and "v3d_recon_bvh_build_nodes" in err() and "null" in err(), k
    assert bn(F=0) == -1 and "num_faces 0" in err()
    assert bn(F=-5) == -1 and "num_faces -5" in err()
    assert bn(F=big) == -1 and "num_faces" in err()
    fr = calls(lib.v3d_recon_bvh_fit_round, ("left", "right", "F", "din", "dout", "lo", "hi", "changed", "stream"),
               left=p, right=p, F=320, din=p, dout=q, lo=p, hi=p, changed=p, stream=None)
    for k in ("left", "right", "din", "dout", "lo", "hi", "changed"):
        assert fr(**{k: None}) == -1 and "v3d_recon_bvh_fit_round" in err() and "null" in err(), k
    assert fr(dout=p) == -1 and "two buffers" in err()
    assert fr(F=1) == -1 and "num_faces 1" in err() and "no internal node" in err()
    assert fr(F=big) == -1 and "num_faces" in err()
    tree = ("left", "right", "order", "lo", "hi", "verts", "V", "faces", "F")
    tree_defaults = dict(left=p, right=p, order=p, lo=p, hi=p, verts=p, V=162, faces=p, F=320)

    def tree_refusals(call, name):
        for k in ("left", "right", "order", "lo", "hi", "verts", "faces"):
            assert call(**{k: None}) == -1 and name in err() and "null" in err(), k
        assert call(V=0) == -1 and "num_verts" in err()
        assert call(F=0) == -1 and "num_faces 0" in err()
        assert call(F=big) == -1 and "num_faces" in err()

    ch = calls(lib.v3d_recon_bvh_closest_hit, ("o", "d", "tmin", "tmax", "N", "cull") + tree + ("t", "face", "uv", "stream"),
               o=p, d=p, tmin=0.0, tmax=1.0, N=100, cull=0, t=p, face=p, uv=p, stream=None, **tree_defaults)
    for k in ("o", "d", "t", "face", "uv"):
        assert ch(**{k: None}) == -1 and "v3d_recon_bvh_closest_hit" in err() and "null" in err(), k
    tree_refusals(ch, "v3d_recon_bvh_closest_hit")
    assert ch(N=0) == -1 and "num_rays" in err()
    assert ch(N=-1) == -1 and "num_rays" in err()
    assert ch(cull=3) == -1 and "cull 3" in err()
    assert ch(cull=-1) == -1 and "cull -1" in err()
    assert ch(tmin=float("nan")) == -1 and "NaN" in err()
    assert ch(tmax=float("nan")) == -1 and "NaN" in err()
    bk = calls(lib.v3d_recon_tex_bake_normals, ("lv", "lV", "lf", "lF", "ln", "R", "md") + tree + ("hn", "owner", "nmap", "dist", "hit", "stream"),
               lv=p, lV=162, lf=p, lF=320, ln=p, R=64, md=0.1, hn=p, owner=p, nmap=p, dist=p, hit=p, stream=None, **tree_defaults)
    for k in ("lv", "lf", "ln", "hn", "owner", "nmap", "dist", "hit"):
        assert bk(**{k: None}) == -1 and "v3d_recon_tex_bake_normals" in err() and "null" in err(), k
    tree_refusals(bk, "v3d_recon_tex_bake_normals")
    assert bk(lV=0) == -1 and "low_num_verts" in err()
    assert bk(lF=0) == -1 and "low_num_faces" in err()
    assert bk(R=0) == -1 and "tex_size 0" in err() and "4096" in err()
    assert bk(R=4097) == -1 and "tex_size 4097" in err()
    assert bk(lF=320, R=51) == -1 and "texture too small for 320 faces" in err()
    assert bk(md=-0.1) == -1 and "max_dist" in err()
    assert bk(md=float("inf")) == -1 and "max_dist" in err()
    assert bk(md=float("nan")) == -1 and "max_dist" in err()


# ---- the restatement's own honesty ----------------------------------------------------------------------------------------------------------
def test_brute_force_on_hand_made_rays():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    f = torch.tensor([[3, 4, 5], [0, 1, 2], [0, 1, 2], [0, 1, 1], [0, 7, 2]])          # z = 1; z = 0 twice; zero area; an index that is no vertex
    o = torch.tensor([[0.25, 0.25, -1.0], [0.25, 0.25, 3.0], [2.0, 2.0, -1.0], [0.25, 0.25, -1.0], [-1.0, 0.25, 0.0]])
    d = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])          # the last: in the plane z = 0
    for dt in (F64, F32):
        r = B.closest_hit(v, f, o, d, 0.0, B.INF, 0, dt)
        assert r["face"].tolist() == [1, 0, -1, -1, -1] and r["t"].tolist() == [0.5, 2.0, B.INF, B.INF, B.INF]          # t in units of d; the tie: face 1
        assert r["uv"][0].tolist() == [0.25, 0.25] and r["uv"][2].tolist() == [0.0, 0.0]
        # Ng = +z on every face: a ray along +z sees Ng . d > 0
        assert B.closest_hit(v, f, o, d, 0.0, B.INF, 2, dt)["face"].tolist() == [1, -1, -1, -1, -1]
        assert B.closest_hit(v, f, o, d, 0.0, B.INF, 1, dt)["face"].tolist() == [-1, 0, -1, -1, -1]
        assert B.closest_hit(v, f, o, d, 0.0, 0.5, 0, dt)["face"].tolist() == [1, -1, -1, -1, -1]                       # t <= tmax is closed
        assert B.closest_hit(v, f, o, d, 0.5, B.INF, 0, dt)["face"].tolist() == [1, 0, -1, -1, -1]                      # tmin <= t is closed
        assert B.closest_hit(v, f, o, d, 0.5, B.INF, 0, dt, open_min=True)["face"].tolist() == [0, 0, -1, -1, -1]       # ... and open on request
        assert B.closest_hit(v, f, o, d, 0.0, 0.25, 0, dt)["face"].tolist() == [-1] * 5                                 # tmax in front of the first hit
    r = B.closest_hit(v, f, o, d, 0.0, B.INF, 0)
    assert r["keep"].tolist() == [False, True, True, True, True]                       # the tie has no margin to its runner-up


def test_tree_checker_accepts_a_right_tree_and_refuses_wrong_ones():
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [2, 1, 0], [4, 0, 1], [5, 0, 1], [4, 1, 2.0]])
    f = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 9, 1]])                     # the last has an index that is no vertex: the empty box
    flo, fhi = B.face_boxes(v, f)
    assert flo[3].tolist() == [B.INF] * 3 and fhi[3].tolist() == [-B.INF] * 3 and flo[2].tolist() == [4, 0, 1] and fhi[2].tolist() == [5, 1, 2]
    # F = 4: internal 0 (root), 1, 2; leaves 3 .. 6 = faces order[0 .. 3]
    order = torch.tensor([3, 0, 1, 2])
    left, right = torch.tensor([1, 3, 5]), torch.tensor([2, 4, 6])
    parent = torch.tensor([-1, 0, 0, 1, 1, 2, 2])
    leaf_lo, leaf_hi = flo[order], fhi[order]
    lo = torch.cat([torch.zeros(3, 3), leaf_lo])
    hi = torch.cat([torch.zeros(3, 3), leaf_hi])
    lo[1], hi[1] = torch.minimum(leaf_lo[0], leaf_lo[1]), torch.maximum(leaf_hi[0], leaf_hi[1])
    lo[2], hi[2] = torch.minimum(leaf_lo[2], leaf_lo[3]), torch.maximum(leaf_hi[2], leaf_hi[3])
    lo[0], hi[0] = torch.minimum(lo[1], lo[2]), torch.maximum(hi[1], hi[2])
    assert hi[1].tolist() == [1, 1, 0]                                                 # the empty box adds nothing
    assert B.check_tree(order, left, right, parent, lo, hi, v, f) == 2
    one = B.face_boxes(v, f[:1])
    assert B.check_tree(torch.tensor([0]), torch.tensor([-1]), torch.tensor([-1]), torch.tensor([-1]), one[0], one[1], v, f[:1]) == 0
    wrong = [dict(left=torch.tensor([1, 3, 3])), dict(parent=torch.tensor([-1, 0, 0, 1, 2, 2, 2])), dict(order=torch.tensor([3, 0, 1, 1])),
             dict(hi=hi + torch.tensor([0.0, 0.0, 1e-6])), dict(left=torch.tensor([1, 0, 5]))]
    for change in wrong:
        args = dict(order=order, left=left, right=right, parent=parent, lo=lo, hi=hi)
        args.update(change)
        with pytest.raises(AssertionError):
            B.check_tree(args["order"], args["left"], args["right"], args["parent"], args["lo"], args["hi"], v, f)
    assert [B.height_bound(F) for F in (1, 2, 3, 257, 2 ** 30)] == [30, 31, 32, 39, 60] and B.height_bound(2 ** 30) < 64


def test_bake_on_an_analytic_sphere_gives_radial_normals():
    """A coarse sphere inside a fine one with exactly radial vertex normals: every texel hits outwards, the distance is the gap between the
    two surfaces, and the baked normal is the direction of the texel's own position to within the fine mesh's facet size."""
    lv, lf = M.icosphere(1, 0.45, seed=2)
    hv, hf = M.icosphere(3, 0.5, seed=1)
    hn = torch.nn.functional.normalize(hv.double(), dim=1).float()
    ln = torch.nn.functional.normalize(lv.double(), dim=1).float()
    R = 64
    b = B.bake(lv, lf, ln, hv, hf, hn, R, 0.2)
    S, _ = TX.layout(lf.shape[0], R)
    assert S == 9 and torch.equal(b["owner"], TX.texel_cells(lf.shape[0], R)[0])
    cast = b["cast"]
    assert torch.equal(cast, b["owner"] >= 0) and int(cast.sum()) > 3000 and bool((b["side"][cast] == 1).all())
    un = ~cast
    assert bool((b["normal"][un] == torch.tensor([0.0, 0.0, 1.0], dtype=F64)).all()) and bool(torch.isnan(b["dist"][un]).all()) and bool((b["hit_face"][un] == -1).all())
    # the texel's own position, restated here: the normal must point along it
    owner, i, j = TX.texel_cells(lf.shape[0], R)
    tri = lf[owner.clamp_min(0)]
    b1 = (i.double() / (S - 3)).clamp(0, 1)
    b2 = torch.minimum((j.double() / (S - 3)).clamp_min(0), 1 - b1)
    P = (1 - b1 - b2)[:, None] * lv.double()[tri[:, 0]] + b1[:, None] * lv.double()[tri[:, 1]] + b2[:, None] * lv.double()[tri[:, 2]]
    # the ray leaves P along the interpolated normal, which is not exactly radial on a flat face: the hit point Q = P + t n is what counts
    n_low = B.unit((1 - b1 - b2)[:, None] * ln.double()[tri[:, 0]] + b1[:, None] * ln.double()[tri[:, 1]] + b2[:, None] * ln.double()[tri[:, 2]])
    Q = P + b["dist"][:, None] * n_low
    radial = torch.nn.functional.normalize(Q[cast], dim=1)
    ang = torch.rad2deg(torch.acos((b["normal"][cast] * radial).sum(1).clamp(-1, 1)))
    gap = b["dist"][cast]
    print(f"{int(cast.sum())} texels: angle to the radius at the hit up to {float(ang.max()):.3e} degrees; |Q| {float(Q[cast].norm(dim=1).min()):.4f} .. "
          f"{float(Q[cast].norm(dim=1).max()):.4f}; distance {float(gap.min()):.4f} .. {float(gap.max()):.4f}")
    assert float(ang.max()) < 0.05                                                     # linear against spherical interpolation over a 4.5-degree facet
    assert 0.495 < float(Q[cast].norm(dim=1).min()) and float(Q[cast].norm(dim=1).max()) <= 0.5 + 1e-7          # on the fine mesh: chords of the sphere
    assert 0.04 < float(gap.min()) and float(gap.max()) < 0.12
    assert float((b["normal"][cast].norm(dim=1) - 1).abs().max()) < 1e-12


# ---- OBJ / MTL / PNG ----------------------------------------------------------------------------------------------------------------------
def test_obj_writer_without_a_normal_map_is_unchanged_and_with_one_round_trips(tmp_path):
    from PIL import Image
    from v3d_amd.recon import mesh_texture as MT
    v, f, c = M.mesh_scene("sphere", 1)
    R = 64
    vt, tex = TX.face_uvs(f.shape[0], R, F32), TX.random_texture(R)
    g = torch.Generator().manual_seed(4)
    nm = torch.nn.functional.normalize(torch.randn(R * R, 3, generator=g), dim=1)
    for d in ("plain", "none", "mapped"):
        os.makedirs(tmp_path / d)
    MT.save_textured_obj(str(tmp_path / "plain" / "m.obj"), v, f, vt, tex)
    MT.save_textured_obj(str(tmp_path / "none" / "m.obj"), v, f, vt, tex, normal_map=None)
    MT.save_textured_obj(str(tmp_path / "mapped" / "m.obj"), v, f, vt, tex, normal_map=nm)
    read = lambda d, n: open(tmp_path / d / n, "rb").read()  # noqa: E731
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "none")) == ["m.mtl", "m.obj", "m.png"]
    assert sorted(os.listdir(tmp_path / "mapped")) == ["m.mtl", "m.obj", "m.png", "m_normal.png"]
    old_mtl = b"newmtl m\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd m.png\n"          # what the writer wrote before the argument existed
    assert read("plain", "m.mtl") == read("none", "m.mtl") == old_mtl and read("mapped", "m.mtl") == old_mtl + b"norm m_normal.png\n"
    for n in ("m.obj", "m.png"):
        assert read("plain", n) == read("none", n) == read("mapped", n), n
    assert read("plain", "m.obj").startswith(b"mtllib m.mtl\nusemtl m\nv ") and np.array_equal(
        np.asarray(Image.open(tmp_path / "plain" / "m.png")).reshape(-1, 3), np.floor(np.clip(tex.numpy(), 0, 1) * 255.0 + 0.5).astype(np.uint8))
    img = np.asarray(Image.open(tmp_path / "mapped" / "m_normal.png"))
    assert img.shape == (R, R, 3) and img.dtype == np.uint8
    enc = 0.5 * nm.numpy().reshape(R, R, 3) + 0.5
    assert np.array_equal(img, np.floor(np.clip(enc, 0, 1) * 255.0 + 0.5).astype(np.uint8))
    assert float(np.abs(img.astype(np.float64) / 255.0 - enc).max()) <= 0.5 / 255 + 1e-7
    rv, rf, rvt, rtex = MT.read_textured_obj(str(tmp_path / "mapped" / "m.obj"))        # the reader ignores the new line
    assert np.array_equal(rv, v.numpy()) and np.array_equal(rf, f.numpy()) and np.array_equal(rvt, vt.numpy()) and rtex.shape == (R * R, 3)
    with pytest.raises(ValueError, match="normal map of 10 texels"):
        MT.save_textured_obj(str(tmp_path / "bad.obj"), v, f, vt, tex, normal_map=torch.zeros(10, 3))


# ---- the script and the host API ----------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_parse():
    mod = _entry("bake_normals")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh_50k.obj", "--high", "out/gs/mesh_clean.ply", "-o", "out/gs/nm.obj"]))
    assert a == {"mesh": "out/gs/mesh_50k.obj", "high": "out/gs/mesh_clean.ply", "out": "out/gs/nm.obj", "white_background": False,
                 "texture_resolution": 1024, "max_dist": None, "views": 18, "reso": 512, "radius": 2.0, "elevation": 0.0, "fov": 60.0, "render_orbit": 0}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov"):
        assert a[k] == recon[k], k
    b = vars(ap.parse_args(["--mesh", "m.ply", "--high", "h.ply", "--texture_resolution", "2048", "--max_dist", "0.01", "--render_orbit", "36", "-w"]))
    assert (b["texture_resolution"], b["max_dist"], b["render_orbit"], b["white_background"], b["out"]) == (2048, 0.01, 36, True, None)
    for bad in (["--high", "h.ply"], ["--mesh", "m.ply"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    base = ["--mesh", "does/not/exist.ply", "--high", "does/not/exist.ply"]
    for bad in (["--texture_resolution", "0"], ["--texture_resolution", "4097"], ["--max_dist", "-1"], ["--max_dist", "inf"], ["--max_dist", "nan"],
                ["-o", "out.ply"], ["--render_orbit", "-1"], ["--views", "-1"], ["--reso", "0"]):
        with pytest.raises(SystemExit):                    # refused before anything is read
            mod.main(base + bad)
    with pytest.raises(SystemExit):
        mod.main(["--mesh", "does/not/exist.glb", "--high", "does/not/exist.ply"])


def test_host_api_refuses_bad_arguments_and_answers_the_empty_low_mesh_without_a_launch():
    from v3d_amd.recon import mesh_bake as MB
    v, f = M.icosphere(0)
    none_f, none_v = torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3)
    for vv, ff in ((v, none_f), (none_v, none_f)):
        with pytest.raises(ValueError, match="nothing to hit"):
            MB.build_bvh(vv, ff, device="cpu")
    with pytest.raises(ValueError, match="integers"):
        MB.build_bvh(v, f.float(), device="cpu")
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        MB.build_bvh(v[:, :2], f, device="cpu")
    with pytest.raises(ValueError, match="not finite"):
        MB.build_bvh(v * float("inf"), f, device="cpu")
    assert MB.height_bound(1) == 30 and MB.height_bound(2) == 31 and MB.height_bound(257) == 39 and MB.height_bound(MB.MAX_FACES) + 8 < 2 * 64
    assert all(MB.height_bound(F) == B.height_bound(F) < 64 for F in (1, 2, 3, 257, 320, 50_000, 161_952, MB.MAX_FACES))
    kw = dict(device="cpu")
    with pytest.raises(ValueError, match="tex_size 0"):
        MB.bake_normal_map(v, f, v, f, tex_size=0, **kw)
    with pytest.raises(ValueError, match="tex_size 5000"):
        MB.bake_normal_map(v, f, v, f, tex_size=5000, **kw)
    with pytest.raises(ValueError, match="texture too small for 20 faces"):
        MB.bake_normal_map(v, f, v, f, tex_size=15, **kw)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            MB.bake_normal_map(v, f, v, f, tex_size=64, max_dist=bad, **kw)
    with pytest.raises(ValueError, match="outside the vertex array"):
        MB.bake_normal_map(v, f + 1, v, f, tex_size=64, **kw)
    with pytest.raises(ValueError, match="outside the vertex array"):
        MB.bake_normal_map(v, f, v, f + 1, tex_size=64, **kw)
    with pytest.raises(ValueError, match="no faces to hit"):
        MB.bake_normal_map(v, f, v, none_f, tex_size=64, **kw)
    bvh = MB.MeshBVH(v, f.int(), *([torch.zeros(1, dtype=torch.int32)] * 4), torch.zeros(1, 3), torch.zeros(1, 3), 0)
    for bad in (3, -1, True, 1.5):
        with pytest.raises(ValueError, match="cull"):
            MB.cast_rays(bvh, v, v, cull=bad)
    with pytest.raises(ValueError, match="NaN"):
        MB.cast_rays(bvh, v, v, tmin=float("nan"))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        MB.cast_rays(bvh, v, v[:5])
    t, face, uv = MB.cast_rays(bvh, none_v, none_v)                                    # no rays: no launch
    assert tuple(t.shape) == (0,) and tuple(face.shape) == (0,) and tuple(uv.shape) == (0, 2)
    assert abs(MB.default_max_dist(torch.tensor([[0.0, 0, 0], [3, 4, 12]])) - 0.05 * 13) < 1e-6
    for lv, lf in ((none_v, none_f), (v, none_f)):
        nm, stats = MB.bake_normal_map(lv, lf, v, f, tex_size=16, **kw)
        assert tuple(nm.shape) == (256, 3) and nm.dtype == F32 and bool((nm == torch.tensor([0.0, 0.0, 1.0])).all())
        assert (stats["hit_plus"], stats["hit_minus"], stats["missed"], stats["owned"], stats["bvh_rounds"]) == (0, 0, 0, 0, 0)


# ---- the premises of the GPU cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", (0, 1, 2))
@pytest.mark.parametrize("kind", ("sphere", "pair"))
def test_premises_of_the_ray_cases(kind, cull):
    """On the restatement alone: at most 2 % of the 1100 rays (1000 random, 100 axis-parallel) are left out by the margins, the float32 brute
    force picks the fp64 face on every ray kept, every prefix the GPU test takes keeps rays, and the case has hits and misses."""
    v, f, o, d, r64, r32 = B.ray_case(kind, cull)
    assert o.shape == (1100, 3) and int(((d != 0).sum(1) == 1).sum()) == B.N_AXIS
    keep, hit = r64["keep"], r64["face"] >= 0
    out = 1.0 - float(keep.float().mean())
    terr = float((r32["t"].double() - r64["t"])[keep & hit].abs().max())
    print(f"{kind} cull {cull}: {int(hit.sum())} of 1100 rays hit, {100 * out:.3f} % left out, float32 t off by up to {terr:.3e}")
    assert out <= B.EXCLUDE_MAX and 300 < int(hit.sum()) < 900
    assert torch.equal(r32["face"][keep], r64["face"][keep]) and terr < 1e-5
    axis = (d != 0).sum(1) == 1
    assert int((hit & axis).sum()) > 10 and int((~hit & axis).sum()) > 10
    for n in B.RAY_COUNTS:
        assert int(keep[:n].sum()) >= 0.98 * n
    if kind == "sphere" and cull:                      # a closed convex surface seen from outside: one front and one back face to a ray
        other = B.ray_case(kind, 3 - cull)[4]
        assert torch.equal(other["face"] >= 0, hit) and bool(((other["t"] - r64["t"])[hit] * (1 if cull == 1 else -1) > 0).all())


@pytest.mark.parametrize("tex", B.BAKE_SIZES)
@pytest.mark.parametrize("name", B.BAKE_CASES)
def test_premises_of_the_bake_cases(name, tex):
    lv, lf, hv, hf, md = B.bake_scene(name)
    ln, hn = C.normals(lv, lf).float(), C.normals(hv, hf).float()
    b64, b32 = B.bake(lv, lf, ln, hv, hf, hn, tex, md), B.bake(lv, lf, ln, hv, hf, hn, tex, md, F32)
    cast, keep = b64["cast"], b64["keep"]
    out = 1.0 - float(keep[cast].float().mean())
    sides = [int((b64["side"][cast] == s).sum()) for s in (1, -1, 0)]
    print(f"{name} R {tex}: {int(cast.sum())} texels cast, {sides} outwards / inwards / missed, {100 * out:.3f} % left out")
    assert (lf.shape[0], hf.shape[0]) == (320, 1280) and TX.layout(320, 64)[0] == 4 and 13 * TX.layout(320, 100)[0] < 100
    assert out <= B.EXCLUDE_MAX
    assert torch.equal(b32["hit_face"][keep], b64["hit_face"][keep]) and torch.equal(b32["side"][keep], b64["side"][keep])
    assert min(sides[:2]) > 0.15 * int(cast.sum())                                    # both signs, in every case
    assert (sides[2] > 0.3 * int(cast.sum())) if name == "short" else sides[2] == 0    # misses where max_dist is shorter than the bump
    assert bool((keep <= cast).all())


def test_nested_icospheres_of_one_seed_are_a_bad_scene():
    """Why the bake scenes rotate the two meshes differently: with one rotation the low mesh's edges project exactly onto the high mesh's
    edges, and most rays fall inside the margins."""
    lv, lf = M.icosphere(1, 0.5, seed=1)
    hv, hf = M.icosphere(3, 0.5, seed=1)
    hv = B.bumped(hv)
    b = B.bake(lv, lf, C.normals(lv, lf).float(), hv, hf, C.normals(hv, hf).float(), 64, 0.2)
    assert 1.0 - float(b["keep"][b["cast"]].float().mean()) > 0.2


def test_restatement_of_the_end_to_end_scene_lowers_the_angle():
    """RESTATEMENT_REDUCTION_DEG of tests/test_mesh_bake_gpu.py is measured here: by how many degrees the baked map lowers the mean angle to
    the high mesh's normals, on the fp64 restatement.  The scene's condition: at least a quarter of the angle before."""
    import test_mesh_bake_gpu as GPU_TESTS
    sc = B.e2e_cpu()
    r = B.e2e_restatement()
    bk = r["bake"]
    sides = [int((bk["side"][bk["cast"]] == s).sum()) for s in (1, -1, 0)]
    print(f"{sc['high'][1].shape[0]} -> {sc['low'][1].shape[0]} faces: mean angle {r['before']:.3f} -> {r['after']:.3f} degrees, reduction "
          f"{r['reduction']:.3f} ({100 * r['reduction'] / r['before']:.1f} %); texels {sides} outwards / inwards / missed")
    assert 1300 < sc["high"][1].shape[0] < 1600 and sc["low"][1].shape[0] in (299, 300) and len(sc["cams"]) == 4
    assert r["reduction"] >= 0.25 * r["before"] > 0
    assert abs(r["reduction"] - GPU_TESTS.RESTATEMENT_REDUCTION_DEG) <= 0.02          # the figure written into the GPU test
    assert sides[2] < 0.01 * sum(sides)
