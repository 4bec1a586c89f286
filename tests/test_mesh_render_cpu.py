"""The mesh rasterizer of libv3d_recon.so (csrc_recon/meshrast.hip, v3d_amd/recon/mesh_render.py, scripts/pub/render_mesh.py) without a GPU:
the header, the ctypes table and the exports agree, bad arguments are refused before any launch, the script's options parse, the torch
restatement (tests/mesh_render_ref.py) is itself honest about the fill rule and about closed meshes, and the scenes of
tests/test_mesh_render_gpu.py keep their decision margins and are what their tests need: the first seed that keeps the margin at every
sub-pixel depth and size, the list shapes of the early-exit and tie scenes, the int64 headroom at the coordinate limit, the last column
and row of the largest images."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_render_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_ENTRIES = {"v3d_recon_mesh_project", "v3d_recon_mesh_face_setup", "v3d_recon_mesh_duplicate_keys", "v3d_recon_mesh_tile_ranges",
                "v3d_recon_mesh_render"}


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


def test_header_signatures_and_exports_agree(lib):
    from v3d_amd.recon import geometry, mesh_render
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert MESH_ENTRIES <= declared and MESH_ENTRIES <= set(geometry.SIGNATURES)
    assert declared == set(geometry.SIGNATURES)
    for name in MESH_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert int(re.search(r"#define V3D_RECON_MESH_MAX_IMAGE (\d+)", hdr).group(1)) == mesh_render.MAX_IMAGE == 4096
    assert int(re.search(r"#define V3D_RECON_MESH_MAX_SUBPIXEL_BITS (\d+)", hdr).group(1)) == mesh_render.MAX_SUBPIXEL_BITS == 8
    assert os.path.exists(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshrast.hip"))


def _camera(W=32, H=32):
    from v3d_amd.recon.rasterize import gs_camera
    return gs_camera(D.cams_for(W, H)[0], [0, 0, 0])


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    cam, wide, high = _camera(), _camera(4097, 32), _camera(32, 4097)
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731
    ref = C.byref
    # project
    assert lib.v3d_recon_mesh_project(None, 8, ref(cam), 8, p, p, p, None) == -1 and "v3d_recon_mesh_project" in err() and "null" in err()
    assert lib.v3d_recon_mesh_project(p, 8, None, 8, p, p, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_mesh_project(p, 8, ref(cam), 8, p, p, None, None) == -1 and "null" in err()
    assert lib.v3d_recon_mesh_project(p, 0, ref(cam), 8, p, p, p, None) == -1 and "positive" in err()
    assert lib.v3d_recon_mesh_project(p, 8, ref(cam), 9, p, p, p, None) == -1 and "subpixel_bits 9" in err()
    assert lib.v3d_recon_mesh_project(p, 8, ref(cam), -1, p, p, p, None) == -1 and "subpixel_bits" in err()
    assert lib.v3d_recon_mesh_project(p, 8, ref(wide), 8, p, p, p, None) == -1 and "4097" in err() and "4096" in err()
    assert lib.v3d_recon_mesh_project(p, 8, ref(high), 8, p, p, p, None) == -1 and "4096" in err()
    # face_setup
    assert lib.v3d_recon_mesh_face_setup(None, 4, p, p, 8, 32, 32, 8, 1, p, p, None) == -1 and "v3d_recon_mesh_face_setup" in err() and "null" in err()
    assert lib.v3d_recon_mesh_face_setup(p, 4, p, p, 8, 32, 32, 8, 1, p, None, None) == -1 and "null" in err()
    assert lib.v3d_recon_mesh_face_setup(p, 0, p, p, 8, 32, 32, 8, 1, p, p, None) == -1 and "positive" in err()
    assert lib.v3d_recon_mesh_face_setup(p, 4, p, p, 0, 32, 32, 8, 1, p, p, None) == -1 and "positive" in err()
    assert lib.v3d_recon_mesh_face_setup(p, 4, p, p, 8, 0, 32, 8, 1, p, p, None) == -1 and "4096" in err()
    assert lib.v3d_recon_mesh_face_setup(p, 4, p, p, 8, 32, 4097, 8, 1, p, p, None) == -1 and "4097" in err()
    assert lib.v3d_recon_mesh_face_setup(p, 4, p, p, 8, 32, 32, 9, 1, p, p, None) == -1 and "subpixel_bits" in err()
    # duplicate_keys
    assert lib.v3d_recon_mesh_duplicate_keys(p, 4, p, 8, p, p, p, 32, 32, 8, None, p, None) == -1 and "v3d_recon_mesh_duplicate_keys" in err()
    assert lib.v3d_recon_mesh_duplicate_keys(p, 4, p, 8, p, None, p, 32, 32, 8, p, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_mesh_duplicate_keys(p, -3, p, 8, p, p, p, 32, 32, 8, p, p, None) == -1 and "positive" in err()
    assert lib.v3d_recon_mesh_duplicate_keys(p, 4, p, 8, p, p, p, 4097, 32, 8, p, p, None) == -1 and "4096" in err()
    assert lib.v3d_recon_mesh_duplicate_keys(p, 4, p, 8, p, p, p, 32, 32, 16, p, p, None) == -1 and "subpixel_bits 16" in err()
    # tile_ranges
    assert lib.v3d_recon_mesh_tile_ranges(p, 4, 32, 32, None, None) == -1 and "v3d_recon_mesh_tile_ranges" in err() and "null" in err()
    assert lib.v3d_recon_mesh_tile_ranges(None, 4, 32, 32, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_mesh_tile_ranges(p, -1, 32, 32, p, None) == -1 and "negative" in err()
    assert lib.v3d_recon_mesh_tile_ranges(p, 4, 32, -2, p, None) == -1 and "4096" in err()
    # render (a null n_hit is legal: it enables the early exit; vals_sorted may be null with empty ranges)
    args = lambda **kw: [kw.get(k, d) for k, d in (("ranges", p), ("vals", p), ("faces", p), ("F", 4), ("pix_q", p), ("zv", p), ("zmin", p),  # noqa: E731
                                                   ("colors", p), ("cam", ref(cam)), ("bits", 8), ("image", p), ("depth", p), ("alpha", p),
                                                   ("face_id", p), ("n_hit", None), ("stream", None))]
    for k in ("ranges", "faces", "pix_q", "zv", "zmin", "colors", "cam", "image", "depth", "alpha", "face_id"):
        assert lib.v3d_recon_mesh_render(*args(**{k: None})) == -1 and "v3d_recon_mesh_render" in err() and "null" in err(), k
    assert lib.v3d_recon_mesh_render(*args(F=0)) == -1 and "positive" in err()
    assert lib.v3d_recon_mesh_render(*args(bits=9)) == -1 and "subpixel_bits" in err()
    assert lib.v3d_recon_mesh_render(*args(cam=ref(wide))) == -1 and "4097" in err()
    assert lib.v3d_recon_mesh_render(*args(cam=ref(high))) == -1 and "4096" in err()


def test_host_api_refuses_bad_meshes_and_views():
    from v3d_amd.recon import mesh_render as MR
    cam = D.cams_for(32, 32)[0]
    v, f = M.icosphere(0)
    c = M.position_colors(v)
    with pytest.raises(ValueError, match="outside the vertex array"):
        MR.render_mesh(cam, v, f + 1, c, [0, 0, 0], device="cpu")
    with pytest.raises(ValueError, match="outside the vertex array"):
        MR.render_mesh(cam, v, f - 1, c, [0, 0, 0], device="cpu")
    with pytest.raises(ValueError, match="colours"):
        MR.render_mesh(cam, v, f, c[:-1], [0, 0, 0], device="cpu")
    with pytest.raises(ValueError, match="integers"):
        MR.render_mesh(cam, v, f.float(), c, [0, 0, 0], device="cpu")
    with pytest.raises(ValueError, match="subpixel_bits"):
        MR.render_mesh(cam, v, f, c, [0, 0, 0], subpixel_bits=9, device="cpu")
    with pytest.raises(ValueError, match="4096"):
        MR.render_mesh(D.cams_for(4112, 32)[0], v, f, c, [0, 0, 0], device="cpu")
    # the empty mesh is the background, without a launch (so it runs here)
    out = MR.render_mesh(D.cams_for(56, 40)[0], np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float32),
                         [0.25, 0.5, 1.0], count_hits=True, device="cpu")
    assert set(out) == {"render", "depth", "alpha", "face_id", "n_hit"} and out["render"].shape == (3, 40, 56)
    assert torch.equal(out["render"][:, 7, 9], torch.tensor([0.25, 0.5, 1.0])) and not out["depth"].any() and not out["alpha"].any()
    assert bool((out["face_id"] == -1).all()) and out["face_id"].dtype == torch.int32 and not out["n_hit"].any()


def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_parse_with_the_reconstructions_defaults():
    ap = _entry("render_mesh").build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh.ply", "-o", "out/gs/mesh_orbit", "--render_orbit", "36", "-w", "--video", "out/000000.npy"]))
    assert a == {"mesh": "out/gs/mesh.ply", "out": "out/gs/mesh_orbit", "white_background": True, "render_orbit": 36, "video": "out/000000.npy",
                 "num_frames": None, "radius": 2.0, "elevation": 0.0, "fov": 60.0, "reso": None, "no_cull": False}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov"):
        assert a[k] == recon[k]
    b = ap.parse_args(["--mesh", "m.ply", "--no_cull", "--reso", "128", "--render_orbit", "4"])
    assert b.no_cull and b.reso == 128 and b.video is None and b.out is None and not b.white_background
    with pytest.raises(SystemExit):
        ap.parse_args(["--render_orbit", "4"])          # --mesh is required


def test_fidelity_file_is_strict_json():
    import json
    mod = _entry("render_mesh")
    fid = {"psnr": [float("inf"), 31.25], "psnr_mean": float("inf"), "coverage": [0.25, 0.5], "odd_hit_pixels": [0, 3]}
    text = json.dumps(mod.strict_json(fid), allow_nan=False)           # (raises on a bare Infinity / NaN token)
    back = json.loads(text)
    assert [float(v) for v in back["psnr"]] == fid["psnr"] and float(back["psnr_mean"]) == float("inf")
    assert back["coverage"] == fid["coverage"] and back["odd_hit_pixels"] == fid["odd_hit_pixels"]


# ---- the restatement's own honesty ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", (False, True), ids=("ccw", "cw"))
@pytest.mark.parametrize("split", (0, 1, 2))
def test_restatement_fill_rule_covers_a_pixel_aligned_grid_once(split, flip):
    W, H = 40, 24
    q, faces, (x0, y0, x1, y1) = M.quad_grid(split=split, flip=flip)
    assert 0 < x0 and x1 < W - 1 and 0 < y0 and y1 < H - 1
    zv = torch.full((q.shape[0],), 2.0)
    out = M.rasterize(q, zv, faces, torch.rand(q.shape[0], 3), W, H, [0, 0, 0], cull=False)
    n = out["n_hit"]
    assert bool((n[y0 + 1:y1, x0 + 1:x1] == 1).all())              # interior pixels, those on shared edges and shared vertices included
    assert int(n.max()) == 1                                       # the outer boundary at most once
    outside = torch.ones(H, W, dtype=torch.bool)
    outside[y0:y1 + 1, x0:x1 + 1] = False
    assert not n[outside].any()
    # top-left: the boundary's top row and left column belong to the grid, its bottom row and right column do not
    assert bool((n[y0, x0:x1] == 1).all()) and bool((n[y0:y1, x0] == 1).all())
    assert not n[y1, x0:x1 + 1].any() and not n[y0:y1 + 1, x1].any()


def test_restatement_sees_a_closed_sphere_as_closed():
    for view in range(4):
        cam = D.cams_for(64, 48)[view]
        v, f, c = M.mesh_scene("sphere", M.SEEDS["sphere"])
        pr = M.project(v, cam)
        both = M.rasterize(pr["pix_q"], pr["zv"], f, c, 64, 48, [1, 1, 1], cull=False)
        front = M.rasterize(pr["pix_q"], pr["zv"], f, c, 64, 48, [1, 1, 1], cull=True)
        assert set(both["n_hit"].reshape(-1).tolist()) == {0, 2}
        assert set(front["n_hit"].reshape(-1).tolist()) == {0, 1}
        assert torch.equal(both["face_id"], front["face_id"]) and torch.equal(both["depth"], front["depth"])      # outward winding: front = nearest
        inward = M.rasterize(pr["pix_q"], pr["zv"], f.flip(1), c, 64, 48, [1, 1, 1], cull=True)
        assert torch.equal(inward["n_hit"] > 0, front["n_hit"] > 0) and bool((inward["depth"] >= front["depth"]).all())     # only the far side is left
        assert bool((inward["depth"] > front["depth"])[front["n_hit"] > 0].all())


def test_projection_restatement_is_the_tsdf_passes():
    import recon_geom_ref as R
    cam = D.cams_for(56, 40)[1]
    p = R.voxel_centres(6, 0.8)
    pr = M.project(p, cam, 8)
    ph = torch.cat([p, torch.ones_like(p[:, :1])], 1)
    hom = ph @ cam.full_proj.double()
    fx = ((hom[:, 0] / (hom[:, 3] + 1e-7) + 1) * 56 - 1) * 0.5
    assert float((pr["pix_f"][:, 0] - fx).abs().max()) <= 1e-12 and float((pr["zv"] - (ph @ cam.world_view.double())[:, 2]).abs().max()) <= 1e-12
    assert torch.equal(pr["pix_q"], torch.round(pr["pix_f"] * 256).long()) and not pr["marked"].any()
    near = M.project(torch.stack([cam.center.double() * 0.95, cam.center.double() * 1.5, torch.tensor([float("nan"), 0, 0], dtype=torch.float64)]), cam)
    assert near["marked"].tolist() == [True, True, True] and bool((near["pix_q"] == M.MARK).all())


# ---- scene margins --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.RASTER_CASES, ids=M.case_id)
def test_scenes_keep_their_depth_margin(case):
    """On every pixel of every parity case the two nearest hits differ in z by Z_GAP_MARGIN at least, and the float32 run of the restatement
    is off by Z_FP32_ERR at most: the kernel's fp32 z then orders every pixel's hits as fp64 does, and no pixel is left out of a comparison."""
    kind, seed, W, H, _, cull = case
    cam = M.case_camera(case)
    v, f, c = M.mesh_scene(kind, seed)
    assert f.shape[0] == (320 if kind == "sphere" else 640)
    pr = M.project(v, cam, 8, torch.float32)            # (the GPU test uses the kernel's own snap; it asserts the margin on that again)
    assert not pr["marked"].any()
    r64 = M.rasterize(pr["pix_q"], pr["zv"], f, c, W, H, [1, 1, 1], cull=cull)
    r32 = M.rasterize(pr["pix_q"], pr["zv"], f, c, W, H, [1, 1, 1], cull=cull, dtype=torch.float32)
    gap, err = float(r64["gap"].min()), float((r32["depth"].double() - r64["depth"]).abs().max())
    print(f"smallest gap {gap:.3e}, float32 restatement z error {err:.3e}")
    assert gap >= M.Z_GAP_MARGIN and err <= M.Z_FP32_ERR
    assert torch.equal(r32["face_id"], r64["face_id"]) and torch.equal(r32["n_hit"], r64["n_hit"])
    assert 0.1 < float(r64["alpha"].mean()) < 0.6                     # a scene: covered and uncovered pixels
    if kind == "pair":
        first = r64["face_id"][(r64["face_id"] >= 0)] < 320
        assert 0.2 < float(first.double().mean()) < 0.8                 # both spheres win pixels: they interpenetrate in the image
    assert M.SEEDS_TRIED[kind] >= 1


def test_layer_stack_and_tie_scene_are_what_the_gpu_test_needs():
    q, zv, faces, colors = M.layer_stack()
    assert faces.shape[0] == 700 > 2 * 256                            # 3 LDS batches in the first tile's list
    out = M.rasterize(q, zv, faces, colors, 56, 40, [0, 0, 0], cull=False)
    assert bool((out["n_hit"][:16, :16] == 700).all()) and int(out["n_hit"].max()) == 700
    assert float(out["gap"].min()) >= 5e-4                            # layers 1e-3 apart, tilted by less than 2e-4
    nearest = int(torch.argmin(zv.reshape(-1, 3).min(1).values))
    assert nearest == 695 and bool((out["face_id"][:16, :16] == nearest).all())          # the nearest layer is in the last batch of face order
    for swap in (False, True):
        q, zv, faces, colors = M.tie_pair(swap=swap)
        out = M.rasterize(q, zv, faces, colors, 64, 48, [0, 0, 0], cull=False)
        hit = out["n_hit"] > 0
        assert int(hit.sum()) > 200 and bool((out["n_hit"][hit] == 2).all()) and float(out["gap"][hit].max()) == 0.0      # bit-equal on purpose
        assert bool((out["face_id"][hit] == 0).all())


def test_undrawn_mesh_is_undrawn_in_the_restatement():
    for view in (0, 2):
        cam = D.cams_for(64, 48)[view]
        v, f, c, names = M.undrawn_mesh(cam)
        pr = M.project(v, cam)
        assert pr["marked"].tolist() == [False, False, True, False, False, True] + [False] * 8
        for cull in (True, False):
            drawn, area2, _, tiles = M.drawn_faces(pr["pix_q"], f, 64, 48, 8, cull)
            assert not drawn.any() and not tiles.any(), [n for n, d in zip(names, drawn.tolist()) if d]
        assert int(area2[2]) != 0 and int(area2[3]) == 0 and int(area2[4]) == 0


# ---- sub-pixel depths and ragged images: the premises of the edge cases ---------------------------------------------------------------
def _edge_restated(case, seed=None):
    kind, s, W, H, view, cull, bits = case
    v, f, c = M.mesh_scene(kind, s if seed is None else seed)
    pr = M.project(v, D.cams_for(W, H)[view], bits, torch.float32)      # (the GPU test uses the kernel's own snap; it asserts the premise on that again)
    return pr, f, c, M.rasterize(pr["pix_q"], pr["zv"], f, c, W, H, [1, 1, 1], bits=bits, cull=cull)


def test_edge_cases_pair_every_bit_depth_with_the_sizes_that_matter():
    assert len(M.EDGE_CASES) == len({M.edge_case_id(c) for c in M.EDGE_CASES}) >= 16
    assert {c[6] for c in M.EDGE_CASES} == set(M.EDGE_BITS) == {0, 1, 4, 7} and {(c[2], c[3]) for c in M.EDGE_CASES} == set(M.EDGE_SIZES)
    assert set(M.EDGE_SIZES) == {(37, 21), (17, 50), (13, 9), (1, 1)}
    for bits in M.EDGE_BITS:
        sizes = {(c[2], c[3]) for c in M.EDGE_CASES if c[6] == bits}
        assert any(W % 2 == 1 or H % 2 == 1 for W, H in sizes if (W, H) != (1, 1)) and any(W < 16 or H < 16 for W, H in sizes)
        assert {c[5] for c in M.EDGE_CASES if c[6] == bits} == {True, False}                 # culling on and off at every bit depth
        assert any(not c[5] and c[2] > 1 for c in M.EDGE_CASES if c[6] == bits)              # a closed scene with culling off: the parity of n_hit
    for size in M.EDGE_SIZES:
        assert len({c[6] for c in M.EDGE_CASES if (c[2], c[3]) == size}) >= 2
    assert {c[0] for c in M.EDGE_CASES} == {"sphere", "pair"}
    assert set(M.REFINE_EDGE_CASES) <= set(M.EDGE_CASES) and {0, 4} <= {c[6] for c in M.REFINE_EDGE_CASES}
    assert all((c[2] % 2 == 1 or c[3] % 2 == 1) for c in M.REFINE_EDGE_CASES)


@pytest.mark.parametrize("case", M.EDGE_CASES, ids=M.edge_case_id)
def test_edge_scenes_keep_their_depth_margin(case):
    """test_scenes_keep_their_depth_margin at 0, 1, 4 and 7 sub-pixel bits on odd images, images below a tile and a single pixel.  The seed
    of a case is the FIRST that keeps the margin on every pixel (every smaller one breaks it); the one case without such a seed up to
    SEED_LIMIT leaves at most EXCLUDE_MAX of its covered pixels out of the comparison of face_id, depth and colour."""
    kind, seed, W, H, _, cull, bits = case
    name = M.edge_case_id(case)
    pr, f, c, r64 = _edge_restated(case)
    assert not pr["marked"].any()
    r32 = M.rasterize(pr["pix_q"], pr["zv"], f, c, W, H, [1, 1, 1], bits=bits, cull=cull, dtype=torch.float32)
    keep, left_out = M.compared_pixels(r64, case)
    covered = int((r64["n_hit"] > 0).sum())
    gap, err = float(r64["gap"][keep].min()), float((r32["depth"].double() - r64["depth"])[keep].abs().max())
    print(f"smallest gap {gap:.3e}, float32 restatement z error {err:.3e}, {covered} of {W * H} pixels covered, {left_out} left out")
    assert gap >= M.Z_GAP_MARGIN and err <= M.Z_FP32_ERR
    assert torch.equal(r32["face_id"][keep], r64["face_id"][keep]) and torch.equal(r32["n_hit"], r64["n_hit"])
    if name in M.EDGE_EXCLUDING:
        assert 0 < left_out <= M.EXCLUDE_MAX * covered and M.EDGE_SEEDS_TRIED[name] == M.SEED_LIMIT
        for s in range(1, M.SEED_LIMIT + 1):                                              # no seed keeps the margin everywhere
            assert float(_edge_restated(case, s)[3]["gap"].min()) < M.Z_GAP_MARGIN, s
    else:
        assert left_out == 0 and M.EDGE_SEEDS_TRIED[name] == seed
        for s in range(1, seed):                                                          # counted up from 1: the smaller seeds break it
            assert float(_edge_restated(case, s)[3]["gap"].min()) < M.Z_GAP_MARGIN, s
    if not cull:
        assert not (r64["n_hit"] % 2 == 1).any()                                          # both scenes are closed, snapped or not
    if (W, H) == (1, 1):
        assert covered == int(M.EDGE_SINGLE_PIXEL_COVERED[bits])
    else:
        assert 0.03 < covered / (W * H) < 0.6 and covered >= 20
        dropped = int(((M.drawn_faces(pr["pix_q"], f, W, H, bits, False)[1] == 0)).sum())
        print(f"{dropped} of {f.shape[0]} faces have no area after the snap")
        if bits <= 1:
            assert dropped >= 5                                                             # the snap flattens faces: the a2 == 0 drop is at work
        if case in M.REFINE_EDGE_CASES:
            assert 0.1 < covered / (W * H) < 0.6                                            # what the refinement's tests ask of a view


# ---- the early exit where it must not fire; a tie across batches ----------------------------------------------------------------------
def _synthetic(builder):
    """The scene of the first seed counted up from 1 whose pixels all keep Z_GAP_MARGIN (TIE_PIXEL apart) in fp64 and decide alike in float32"""
    for seed in range(1, M.SEED_LIMIT + 1):
        q, zv, faces, colors = builder(seed=seed)
        r64 = M.rasterize(q, zv, faces, colors, 56, 40, [0, 0, 0], cull=False)
        r32 = M.rasterize(q, zv, faces, colors, 56, 40, [0, 0, 0], cull=False, dtype=torch.float32)
        gap = r64["gap"].clone()
        if builder is M.tie_across_batches:
            gap[M.TIE_PIXEL[1], M.TIE_PIXEL[0]] = float("inf")
        if float(gap.min()) >= M.Z_GAP_MARGIN and torch.equal(r32["face_id"], r64["face_id"]):
            return seed, q, zv, faces, colors, r64, r32
    raise AssertionError("no seed keeps the margin")


def test_steep_cover_keeps_the_early_exit_from_firing():
    seed, q, zv, faces, colors, r64, r32 = _synthetic(M.steep_cover)
    assert seed == M.SYNTH_SEEDS["steep_cover"] == M.SYNTH_SEEDS_TRIED["steep_cover"]
    F = faces.shape[0]
    assert F == 1 + M.STEEP_FILLERS + M.STEEP_LAYERS < 1000 and bool(r64["drawn"].all())
    zmin = zv[faces].min(1).values
    first_layer = 1 + M.STEEP_FILLERS
    assert float(zmin[0]) == 1.0 and bool((zmin[1:first_layer] > 1.0).all()) and bool((zmin[1:first_layer] < 2.0).all())
    assert zmin[first_layer:].tolist() == pytest.approx([2.0 + 0.1 * k for k in range(M.STEEP_LAYERS)])
    assert bool((r64["tiles"][1:first_layer] == 1).all())                         # every filler lies in one tile
    idx, zsorted = M.tile_list(q, zv, faces, 56, 40)
    assert idx.numel() == F > 2 * 256 and int(idx[0]) == 0 and bool((zsorted[1:] >= zsorted[:-1]).all())
    pos = int(torch.nonzero(idx == first_layer)[0])
    assert pos == first_layer >= 2 * 256 and set(idx[:pos].tolist()) == set(range(first_layer))       # in the third batch, behind face 0 and every filler
    for batches in (1, 2):                                                        # every pixel of the tile is covered when batch 2 and batch 3 begin
        head = M.rasterize(q, zv, faces[idx[:256 * batches]], colors, 56, 40, [0, 0, 0], cull=False)
        assert bool((head["n_hit"][:16, :16] > 0).all())
        assert int((head["depth"][:16, :16] >= float(zsorted[256 * batches])).sum()) > 50            # .. and not all in front of the batch's first zmin
    tile = r64["face_id"][:16, :16]
    only0 = M.rasterize(q, zv, faces[:1], colors, 56, 40, [0, 0, 0], cull=False)["depth"][:16, :16]
    won = tile == first_layer
    assert int(won.sum()) > 50 and bool((only0[won] > 2.0).all()) and int((tile == 0).sum()) > 50 and int(((tile > 0) & (tile < first_layer)).sum()) > 50
    assert bool((r64["n_hit"][:16, :16] >= 1 + M.STEEP_LAYERS).all())


def test_tie_across_batches_is_a_tie_in_float32_and_straddles_a_batch():
    seed, q, zv, faces, colors, r64, r32 = _synthetic(M.tie_across_batches)
    assert seed == M.SYNTH_SEEDS["tie_across_batches"] == M.SYNTH_SEEDS_TRIED["tie_across_batches"]
    x, y = M.TIE_PIXEL
    F = faces.shape[0]
    assert F == 2 + M.TIE_FILLERS < 1000 and bool(r64["drawn"].all())
    for r in (r64, r32):
        two = M.rasterize(q, zv, faces[:2], colors, 56, 40, [0, 0, 0], cull=False, dtype=r["depth"].dtype)
        assert int(two["n_hit"][y, x]) == 2 and float(two["gap"][y, x]) == 0.0 and float(two["depth"][y, x]) == 2.0       # both cover it, bit-equal
        each = [M.rasterize(q, zv, faces[k:k + 1], colors, 56, 40, [0, 0, 0], cull=False, dtype=r["depth"].dtype) for k in (0, 1)]
        assert float(each[0]["depth"][y, x]) == float(each[1]["depth"][y, x]) == 2.0
        assert int(r["n_hit"][y, x]) == 2 and int(r["face_id"][y, x]) == 0 and float(r["depth"][y, x]) == 2.0             # no filler covers it
        assert int((r["gap"] == 0).sum()) == 1                                                                            # the only tie
    zmin = zv[faces].min(1).values
    assert float(zmin[0]) == 2.0 and float(zmin[1]) == 1.5 and bool((zmin[2:] > 1.5).all()) and bool((zmin[2:] < 2.0).all())
    idx, zsorted = M.tile_list(q, zv, faces, 56, 40)
    p0, p1 = int(torch.nonzero(idx == 0)[0]), int(torch.nonzero(idx == 1)[0])
    assert p1 == 0 and p0 == 2 * 256 == F - 1 and p0 - p1 - 1 >= 256              # the lower index later, 511 fillers and two batch boundaries between
    assert float(zsorted[p0 - p0 % 256]) == 2.0                                   # its batch's first zmin EQUALS the depth the pixel holds: < or <= decides
    # when that batch begins every pixel of the tile holds a depth at or in front of 2.0: an exit on <= would leave face 1 on the pixel
    head = M.rasterize(q, zv, faces[idx[:p0]], colors, 56, 40, [0, 0, 0], cull=False, dtype=torch.float32)
    assert bool((head["n_hit"][:16, :16] > 0).all()) and float(head["depth"][:16, :16].max()) == 2.0 and int(head["face_id"][y, x]) == 0      # (row 0 of the subset: face 1)
    assert int(idx[0]) == 1


def test_limit_triangle_stays_inside_int64():
    W, H = 56, 40
    q, zv, faces, colors = M.limit_triangle()
    assert int(q[:3].abs().max()) == M.Q_EXTREME == 2 ** 28 - 3 and float(q[:3].abs().max()) < M.Q_LIMIT
    assert len(set(zv[:3].tolist())) == 3
    top = M.edge_intermediates_max(q, faces, W, H, 8)
    assert 2 ** 57 < top < 2 ** 62
    # the restatement's int64 tensors agree with unbounded integers on a corner pixel
    r64 = M.rasterize(q, zv, faces, colors, W, H, [0, 0, 0], cull=False)
    r32 = M.rasterize(q, zv, faces, colors, W, H, [0, 0, 0], cull=False, dtype=torch.float32)
    assert bool(r64["drawn"].all()) and r64["tiles"].tolist() == [12, 9]
    assert bool((r64["n_hit"] >= 1).all()) and set(r64["n_hit"].reshape(-1).tolist()) == {1, 2}      # face 0 holds the whole image, face 1 part of it
    assert 100 < int((r64["face_id"] == 1).sum()) < W * H // 2 and torch.equal(r32["face_id"], r64["face_id"])
    assert float(r64["gap"].min()) >= M.Z_GAP_MARGIN
    far = r64["depth"][r64["face_id"] == 0]
    assert float(far.max()) - float(far.min()) > 1e-5                                                # unequal corner depths show, if only just
    a, b, c = (tuple(int(x) for x in q[i]) for i in range(3))
    exact = ((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
    assert int(M.drawn_faces(q, faces, W, H, 8, False)[1][0]) == exact and abs(exact) > 2 ** 57


@pytest.mark.parametrize("cull", (True, False), ids=("cull", "nocull"))
@pytest.mark.parametrize("size", M.LIMIT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_limit_scenes_reach_the_last_column_and_row(size, cull):
    W, H = size
    assert max(W, H) == 4096
    seed = M.LIMIT_SEEDS[size]
    assert M.LIMIT_SEEDS_TRIED[size] == seed == 1
    v, f, c = M.mesh_scene("pair", seed)
    pr = M.project(v, D.cams_for(W, H)[M.LIMIT_VIEW], 8, torch.float32)
    assert not pr["marked"].any()
    q, zv, ff, cc = M.with_extra(pr["pix_q"], pr["zv"], f, c, M.limit_extra(W, H))
    r64 = M.rasterize(q, zv, ff, cc, W, H, [0, 0, 0], cull=cull)
    r32 = M.rasterize(q, zv, ff, cc, W, H, [0, 0, 0], cull=cull, dtype=torch.float32)
    F = f.shape[0]
    assert bool(r64["drawn"][F:].all()) and int(r64["drawn"][:F].sum()) >= 30                       # the hand-placed faces and a slice of the pair
    last = r64["face_id"][:, -1] if W > H else r64["face_id"][-1, :]
    assert bool((last == F).any())                                                                  # the last column / row is covered
    ys, xs = torch.nonzero(r64["face_id"] == F + 2, as_tuple=True)
    assert (xs if W > H else ys).div(16, rounding_mode="floor").unique().numel() >= 100             # the long face wins pixels in 100 tiles and more
    assert int(r64["face_id"][0, 0]) == F + 1
    pair_ids = r64["face_id"][(r64["face_id"] >= 0) & (r64["face_id"] < F)]
    assert pair_ids.numel() >= (1000 if W > H else 30) and pair_ids.unique().numel() >= 20            # (upright, the pair is 8 pixels across)
    assert int(r64["tiles"][F + 2]) == 256                                                          # the long face is in every tile's list
    gap, err = float(r64["gap"].min()), float((r32["depth"].double() - r64["depth"]).abs().max())
    print(f"smallest gap {gap:.3e}, float32 restatement z error {err:.3e}, {int((r64['n_hit'] > 0).sum())} pixels covered")
    assert gap >= M.Z_GAP_MARGIN and torch.equal(r32["face_id"], r64["face_id"]) and torch.equal(r32["n_hit"], r64["n_hit"])
    assert M.edge_intermediates_max(q, ff[r64["drawn"]], W, H, 8) < 2 ** 62
