"""The gfx950 mesh rasterizer (csrc_recon/meshrast.hip, v3d_amd/recon/mesh_render.py, scripts/pub/render_mesh.py) against the torch restatement
(tests/mesh_render_ref.py): projection, rasterization parity on closed and interpenetrating meshes, the fill rule, tile lists of several
batches with and without the early exit, bit-equal depths, culling and the faces that are not drawn, the project's own extracted mesh, and
the entry point; then the same parity at 0, 1, 4 and 7 sub-pixel bits on odd images, images below one tile and a single pixel, guard
elements around every output of a ragged image, a list whose early exit must NOT fire, a bit-equal depth across a batch boundary, corners
at the 2^28 coordinate limit, 4096 x 16 and 16 x 4096 images, and faces whose indices lie outside the vertex array.  The rasterizing
restatement is fed the KERNEL'S OWN snapped positions and view z, so coverage is exact or it is wrong; the decision margins and the
premises of the scenes are held on the CPU (tests/test_mesh_render_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_render_ref as M
import recon_geom_ref as R
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_render as MR
from v3d_amd.recon.rasterize import gs_camera

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = [0.25, 0.5, 1.0]


def raster(W, H, pix_q, zv, faces, colors, cull, count_hits, bg=BG, bits=8):
    """rasterize_projected on host tensors of snapped positions and view z (the projection bypassed), outputs on the host"""
    gc = gs_camera(D.cams_for(W, H)[0], bg)
    out = MR.rasterize_projected(gc, faces.to(DEV, torch.int32).contiguous(), pix_q.to(DEV, torch.int32).contiguous(), zv.to(DEV, torch.float32),
                                 colors.to(DEV, torch.float32).contiguous(), cull, count_hits, bits)
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def assert_same_decisions(out, ref, n_hit=True):
    assert torch.equal(out["face_id"].long(), ref["face_id"]), f"face_id differs on {int((out['face_id'].long() != ref['face_id']).sum())} pixels"
    assert torch.equal(out["alpha"].double(), ref["alpha"])
    if n_hit:
        assert torch.equal(out["n_hit"].long(), ref["n_hit"]), f"n_hit differs on {int((out['n_hit'].long() != ref['n_hit']).sum())} pixels"


# ---- 1. projection --------------------------------------------------------------------------------------------------------------------
def check_projection(W, H, bits, name):
    cam = D.cams_for(W, H)[2]
    v, _, _ = M.mesh_scene("pair", M.SEEDS["pair"])
    extra, _, _, _ = M.undrawn_mesh(cam)                   # vertices at z <= 0.2, behind the camera and far outside the image
    v = torch.cat([v, extra, torch.tensor([[float("nan"), 0.0, 0.0], [float("inf"), 0.0, 0.0]])])
    zv, pix_f, pix_q = (t.cpu() for t in MR.project_vertices(gs_camera(cam, BG), v.to(DEV), bits))
    r64, r32 = M.project(v, cam, bits), M.project(v, cam, bits, dtype=torch.float32)
    assert torch.equal(pix_q[:, 0] == M.MARK, r64["marked"]) and torch.equal(pix_q[:, 1] == M.MARK, r64["marked"])       # marked: exactly these
    assert int(r64["marked"].sum()) >= 4
    ok = ~r64["marked"]
    perr, zerr = float((pix_f.double() - r64["pix_f"])[ok].abs().max()), float((zv.double() - r64["zv"])[ok].abs().max())
    perr32, zerr32 = float((r32["pix_f"].double() - r64["pix_f"])[ok].abs().max()), float((r32["zv"].double() - r64["zv"])[ok].abs().max())
    qerr = int((pix_q.long() - r64["pix_q"])[ok].abs().max())
    print(f"pix_f {perr:.3e} (float32 restatement {perr32:.3e})  zv {zerr:.3e} ({zerr32:.3e})  pix_q off by at most {qerr} steps")
    record_parity(name, {"pix_f_max_abs": perr, "pix_f_float32_restatement": perr32, "zv_max_abs": zerr, "zv_float32_restatement": zerr32,
                         "pix_q_max_steps": qerr})
    assert perr <= 4 * perr32 and zerr <= 4 * zerr32            # (the compiler may contract to fused multiply-adds: the Chamfer test's allowance)
    assert qerr <= 1


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_projection_matches_the_fp64_restatement(size):
    W, H = size
    check_projection(W, H, 8, f"mesh_render_project[{W}x{H}]")


EDGE_PROJECTIONS = tuple(sorted({(c[2], c[3], c[6]) for c in M.EDGE_CASES}))


@pytest.mark.parametrize("shape", EDGE_PROJECTIONS, ids=lambda s: f"{s[0]}x{s[1]}-b{s[2]}")
def test_projection_matches_the_fp64_restatement_at_every_bit_depth(shape):
    W, H, bits = shape
    check_projection(W, H, bits, f"mesh_render_project[{W}x{H}-b{bits}]")


# ---- 2. rasterization parity ----------------------------------------------------------------------------------------------------------
def check_rasterization(case):
    kind, seed, W, H, _, cull = case[:6]
    bits = M.case_bits(case)
    cam = M.case_camera(case)
    v, f, c = M.mesh_scene(kind, seed)
    out = MR.render_mesh(cam, v, f, c, BG, cull=cull, count_hits=True, subpixel_bits=bits)
    again = MR.render_mesh(cam, v, f, c, BG, cull=cull, count_hits=True, subpixel_bits=bits)
    assert set(out) == {"render", "depth", "alpha", "face_id", "n_hit"} and out["render"].shape == (3, H, W) and out["depth"].shape == (H, W)
    for k in out:
        assert torch.equal(out[k], again[k]), f"{k} differs between two runs"
    zv, _, pix_q = (t.cpu() for t in MR.project_vertices(gs_camera(cam, BG), v.to(DEV), bits))
    ref = M.rasterize(pix_q, zv, f, c, W, H, BG, bits=bits, cull=cull)
    ref32 = M.rasterize(pix_q, zv, f, c, W, H, BG, bits=bits, cull=cull, dtype=torch.float32)
    # the CPU test's margin, on the kernel's own snap: on every pixel, but for the one case that may leave out EXCLUDE_MAX of the covered ones
    keep, left_out = M.compared_pixels(ref, case)
    covered = int((ref["n_hit"] > 0).sum())
    assert float(ref["gap"][keep].min()) >= M.Z_GAP_MARGIN and left_out <= M.EXCLUDE_MAX * covered
    out = {k: t.cpu() for k, t in out.items()}
    err = lambda a, b: float((a.double() - b)[..., keep].abs().max())  # noqa: E731
    derr, ierr = err(out["depth"], ref["depth"]), err(out["render"], ref["image"])
    derr32, ierr32 = err(ref32["depth"], ref["depth"]), err(ref32["image"], ref["image"])
    print(f"depth {derr:.3e} (float32 restatement {derr32:.3e})  image {ierr:.3e} ({ierr32:.3e})  {covered} pixels covered, {left_out} left out")
    record_parity(f"mesh_render_raster[{M.any_case_id(case)}]", {"depth_max_abs": derr, "depth_float32_restatement": derr32, "image_max_abs": ierr,
                                                                  "image_float32_restatement": ierr32, "covered": float(ref["alpha"].mean()),
                                                                  **({"subpixel_bits": bits, "left_out": left_out} if len(case) > 6 else {})})
    # face_id on the compared pixels (all of them, but for that one case); alpha and n_hit on every pixel
    assert_same_decisions(dict(out, face_id=torch.where(keep, out["face_id"].long(), ref["face_id"])), ref)
    assert derr <= 4 * derr32 and ierr <= 4 * ierr32
    # without the hit count (the early exit enabled) the view is the same, bit for bit
    fast = MR.render_mesh(cam, v, f, c, BG, cull=cull, subpixel_bits=bits)
    assert set(fast) == {"render", "depth", "alpha", "face_id"}
    for k in fast:
        assert torch.equal(fast[k].cpu(), out[k]), f"{k} differs with the early exit"
    return out, ref


@pytest.mark.parametrize("case", M.RASTER_CASES, ids=M.case_id)
def test_rasterization_matches_the_restatement(case):
    check_rasterization(case)


@pytest.mark.parametrize("case", M.EDGE_CASES, ids=M.edge_case_id)
def test_rasterization_matches_the_restatement_at_every_bit_depth(case):
    """0, 1, 4 and 7 sub-pixel bits on odd images, images below one tile and a single pixel"""
    _, _, W, H, _, cull, bits = case
    out, ref = check_rasterization(case)
    if not cull:                                               # both scenes are closed; this does not rest on the restatement
        assert int((out["n_hit"] % 2 == 1).sum()) == 0
    if (W, H) == (1, 1):
        assert int(out["alpha"].sum()) == int(M.EDGE_SINGLE_PIXEL_COVERED[bits])
    else:
        assert int(out["alpha"].sum()) >= 20


# ---- 3. fill rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", (False, True), ids=("ccw", "cw"))
@pytest.mark.parametrize("split", (0, 1, 2))
def test_fill_rule_covers_a_pixel_aligned_grid_once(split, flip):
    W, H = 56, 40
    q, faces, (x0, y0, x1, y1) = M.quad_grid(split=split, flip=flip)
    zv = torch.full((q.shape[0],), 2.0)
    colors = torch.rand(q.shape[0], 3, generator=torch.Generator().manual_seed(1))
    out = raster(W, H, q, zv, faces, colors, False, True)
    assert bool((out["n_hit"][y0 + 1:y1, x0 + 1:x1] == 1).all()), "an interior pixel (shared edges and vertices included) is not covered once"
    assert_same_decisions(out, M.rasterize(q, zv, faces, colors, W, H, BG, cull=False))
    assert int(out["n_hit"].max()) == 1


# ---- 4. long lists and the early exit -------------------------------------------------------------------------------------------------
def test_long_lists_with_and_without_the_early_exit():
    W, H = 56, 40
    q, zv, faces, colors = M.layer_stack()
    ref = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False)
    ref32 = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False, dtype=torch.float32)
    counted, fast = raster(W, H, q, zv, faces, colors, False, True), raster(W, H, q, zv, faces, colors, False, False)
    assert int((counted["ranges"][:, 1] - counted["ranges"][:, 0]).max()) == M.LAYERS > 2 * 256          # 3 batches
    assert "n_hit" not in fast
    for k in ("face_id", "depth", "render", "alpha"):
        assert torch.equal(counted[k], fast[k]), f"{k} differs between the counted walk and the early exit"
    assert_same_decisions(counted, ref)
    assert bool((counted["n_hit"][:16, :16] == M.LAYERS).all())
    derr, ierr = float((counted["depth"].double() - ref["depth"]).abs().max()), float((counted["render"].double() - ref["image"]).abs().max())
    derr32, ierr32 = float((ref32["depth"].double() - ref["depth"]).abs().max()), float((ref32["image"].double() - ref["image"]).abs().max())
    print(f"depth {derr:.3e} (float32 restatement {derr32:.3e})  image {ierr:.3e} ({ierr32:.3e})")
    record_parity("mesh_render_layers", {"depth_max_abs": derr, "depth_float32_restatement": derr32, "image_max_abs": ierr,
                                         "image_float32_restatement": ierr32})
    assert derr <= 4 * derr32 and ierr <= 4 * ierr32


# ---- 5. ties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", (False, True), ids=("red-first", "blue-first"))
@pytest.mark.parametrize("count_hits", (False, True), ids=("early-exit", "counted"))
def test_lower_face_index_wins_a_bit_equal_depth(swap, count_hits):
    W, H = 64, 48
    q, zv, faces, colors = M.tie_pair(swap=swap)
    ref = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False)
    out = raster(W, H, q, zv, faces, colors, False, count_hits)
    hit = ref["n_hit"] > 0
    assert int(hit.sum()) > 200
    assert bool((out["face_id"][hit] == 0).all()) and bool((out["face_id"][~hit] == -1).all())
    assert_same_decisions(out, ref, n_hit=count_hits)
    first = out["render"][:, hit]
    assert bool((first[2] > first[0]).all()) if swap else bool((first[0] > first[2]).all())          # the colour of whichever face came first


# ---- 6. culling and dropping ----------------------------------------------------------------------------------------------------------
def assert_empty(out, H, W, bg=BG):
    assert torch.equal(out["render"].cpu(), torch.tensor(bg).view(3, 1, 1).expand(3, H, W))
    assert not out["depth"].any() and not out["alpha"].any() and bool((out["face_id"] == -1).all())
    if "n_hit" in out:
        assert not out["n_hit"].any()


def test_culling_and_faces_that_are_not_drawn():
    W, H = 56, 40
    cam = D.cams_for(W, H)[1]
    v, f, c = M.mesh_scene("sphere", M.SEEDS["sphere"])
    on, off = MR.render_mesh(cam, v, f, c, BG, cull=True), MR.render_mesh(cam, v, f, c, BG, cull=False)
    for k in on:
        assert torch.equal(on[k], off[k]), f"{k}: a closed outward-wound mesh renders differently with culling"
    assert float(on["alpha"].mean()) > 0.1
    # The inward-wound copy.  Of a CLOSED mesh every covered pixel sees as many faces that look away as faces that look at the camera, so
    # reversing the winding cannot empty the view: culling then leaves the far side.  What it removes is every face the outward copy drew:
    # the inward-wound copy of the half that looks at the camera renders as the background.
    gc = gs_camera(cam, BG)
    zv, _, pix_q = MR.project_vertices(gc, v.to(DEV))
    facing = (MR.rasterize_projected(gc, f.to(DEV, torch.int32), pix_q, zv, c.to(DEV), True)["tiles_touched"] > 0).cpu()
    assert 80 < int(facing.sum()) < 200 and set(on["face_id"][on["face_id"] >= 0].unique().tolist()) <= set(torch.nonzero(facing).reshape(-1).tolist())
    assert_empty(MR.render_mesh(cam, v, f[facing].flip(1), c, BG, cull=True, count_hits=True), H, W)
    inward = MR.render_mesh(cam, v, f.flip(1), c, BG, cull=True, count_hits=True)
    ref = M.rasterize(pix_q.cpu(), zv.cpu(), f.flip(1), c, W, H, BG, cull=True)
    assert_same_decisions({k: t.cpu() for k, t in inward.items()}, ref)
    covered = on["alpha"] > 0
    assert torch.equal(inward["alpha"], on["alpha"]) and bool((inward["depth"] > on["depth"])[covered].all())      # the far side only
    assert not facing[inward["face_id"][covered].long().cpu()].any()
    uv, uf, uc, names = M.undrawn_mesh(cam)
    for cull in (True, False):
        assert_empty(MR.render_mesh(cam, uv, uf, uc, BG, cull=cull, count_hits=True), H, W)               # a mesh of undrawn faces only
    zv, _, pix_q = MR.project_vertices(gc, uv.to(DEV))
    full = MR.rasterize_projected(gc, uf.to(DEV, torch.int32), pix_q, zv, uc.to(DEV), False, True)
    assert full["n_inst"] == 0 and not full["tiles_touched"].any() and not full["ranges"].any(), names
    # beside a sphere they change nothing
    both = MR.render_mesh(cam, torch.cat([v, uv]), torch.cat([f, uf + v.shape[0]]), torch.cat([c, uc]), BG, cull=False, count_hits=True)
    for k in off:
        assert torch.equal(both[k], off[k]), k
    assert_empty(MR.render_mesh(cam, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3), BG, count_hits=True), H, W)


# ---- 7. the project's own mesh --------------------------------------------------------------------------------------------------------
def test_extracted_sphere_is_closed_from_every_camera():
    N, bound, r, S = 24, 1.0, 0.5, 64
    ref = R.sphere_volume(N, bound, r)
    f32 = lambda t, *s: t.float().reshape(*s).contiguous().to(DEV)  # noqa: E731
    vol = G.TsdfVolume(N, ref["bound"], ref["trunc"], f32(ref["tsdf_sum"], N, N, N), f32(ref["weight"], N, N, N), f32(ref["rgb_sum"], 3, N, N, N),
                       f32(ref["rgb_weight"], N, N, N))
    verts, faces, colors = G.extract_mesh(vol)
    assert faces.shape[0] > 100
    cams = D.cams_for(S, S, n=4, elevation=15.0)
    renders = []
    for cam in cams:
        off = MR.render_mesh(cam, verts, faces, colors, BG, cull=False, count_hits=True)
        on = MR.render_mesh(cam, verts, faces, colors, BG, cull=True)
        assert int((off["n_hit"] % 2 == 1).sum()) == 0 and int(off["n_hit"].max()) >= 2       # (a voxelised sphere is not convex: 4 at a bump on the rim)
        for k in on:
            assert torch.equal(on[k], off[k]), f"{k}: culling changes the render of the extracted mesh (its winding is not outward)"
        # the image centre lies between the four middle pixels: each sees the sphere's near pole, radius - r away, within a voxel
        mid = on["depth"][S // 2 - 1:S // 2 + 1, S // 2 - 1:S // 2 + 1]
        assert float((mid - (2.0 - r)).abs().max()) <= 2 * bound / N
        renders.append(on["render"])
    fid = MR.mesh_fidelity(verts, faces, colors, cams, torch.stack(renders), BG)
    assert set(fid) == {"psnr", "psnr_mean", "coverage", "odd_hit_pixels"}
    assert fid["psnr"] == [float("inf")] * 4 and fid["psnr_mean"] == float("inf") and fid["odd_hit_pixels"] == [0] * 4
    assert all(0.1 < cv < 0.5 for cv in fid["coverage"])


# ---- 8. entry point -------------------------------------------------------------------------------------------------------------------
def test_render_mesh_script_writes_frames_and_fidelity(tmp_path):
    v, f, c = M.mesh_scene("sphere", M.SEEDS["sphere"])
    ply = str(tmp_path / "mesh.ply")
    G.save_mesh_ply(ply, v, f.to(torch.int32), c)
    rv, rf, rc = G.read_mesh_ply(ply)
    video = MR.render_mesh_orbit(rv, rf, rc.astype(np.float32) / 255.0, 3, 2.0, 0.0, 60.0, 64, True)
    assert video.shape == (3, 64, 64, 3) and video.dtype == np.uint8
    np.save(str(tmp_path / "video.npy"), video)
    out = str(tmp_path / "orbit")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pub", "render_mesh.py"), "--mesh", ply, "-o", out, "--render_orbit", "3", "-w",
                        "--reso", "64", "--video", str(tmp_path / "video.npy")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PSNR mean" in r.stdout and "worst view" in r.stdout and "coverage" in r.stdout
    assert sorted(os.listdir(out)) == ["000.png", "001.png", "002.png", "fidelity.json", "orbit.npy"]
    assert np.array_equal(np.load(os.path.join(out, "orbit.npy")), video)
    fid = json.load(open(os.path.join(out, "fidelity.json")))
    assert set(fid) == {"psnr", "psnr_mean", "coverage", "odd_hit_pixels"} and len(fid["psnr"]) == 3
    assert min(fid["psnr"]) > 40 and fid["odd_hit_pixels"] == [0, 0, 0] and all(0.1 < cv < 0.5 for cv in fid["coverage"])       # 8-bit frames of itself


# ---- 9. nothing is written outside a ragged image -------------------------------------------------------------------------------------
GUARD = 4096
SENTINEL = {torch.float32: 12345.0, torch.int32: 424242}
PREFILL = {torch.float32: float("nan"), torch.int32: -7}


def guarded(n, dtype):
    """A buffer of GUARD sentinels, n prefilled elements (NaN, or -7 for integers) and GUARD sentinels, and the address of the middle part"""
    buf = torch.full((GUARD + n + GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = PREFILL[dtype]
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def assert_guards_untouched(buf, n, name):
    """-> the middle part, on the host: every guard still holds the sentinel and every element between them was overwritten"""
    host = buf.cpu()
    assert bool((host[:GUARD] == SENTINEL[buf.dtype]).all()), f"{name}: a store in front of the buffer"
    assert bool((host[GUARD + n:] == SENTINEL[buf.dtype]).all()), f"{name}: a store past the end of the buffer"
    body = host[GUARD:GUARD + n]
    left = torch.isnan(body) if buf.dtype == torch.float32 else body == PREFILL[buf.dtype]
    assert not left.any(), f"{name}: {int(left.sum())} elements of the image were not written"
    return body


def binned(gc, faces, pix_q, zv, cull, bits):
    """(ranges, vals_sorted, zmin) of the binning, as rasterize_projected builds them (it does not return the sorted list)"""
    from v3d_amd.ops import get_ops
    lib, ops = G.load_library(), get_ops()
    W, H, F, V = int(gc.width), int(gc.height), faces.shape[0], zv.shape[0]
    tiles, zmin = torch.empty(F, dtype=torch.int32, device=DEV), torch.empty(F, dtype=torch.float32, device=DEV)
    assert lib.v3d_recon_mesh_face_setup(faces.data_ptr(), F, pix_q.data_ptr(), zv.data_ptr(), V, W, H, bits, int(cull), tiles.data_ptr(), zmin.data_ptr(),
                                         None) == 0
    offsets = ops.gs_scan(tiles)
    n = int(offsets[-1].item())
    assert n > 0
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    keys, vals = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    assert lib.v3d_recon_mesh_duplicate_keys(faces.data_ptr(), F, pix_q.data_ptr(), V, tiles.data_ptr(), offsets.data_ptr(), zmin.data_ptr(), W, H, bits,
                                             keys.data_ptr(), vals.data_ptr(), None) == 0
    keys_s, vals_s = ops.gs_radix_sort_pairs(keys, vals, 32 + max(1, (ntiles - 1).bit_length()))
    ranges = torch.empty(ntiles, 2, dtype=torch.int32, device=DEV)
    assert lib.v3d_recon_mesh_tile_ranges(keys_s.data_ptr(), n, W, H, ranges.data_ptr(), None) == 0
    return ranges, vals_s, zmin


@pytest.mark.parametrize("case", (M.EDGE_CASES[9], M.EDGE_CASES[3]), ids=M.edge_case_id)
def test_nothing_is_written_outside_a_ragged_image(case):
    """The render and the pixel-weight kernels through the library handle, into buffers with GUARD sentinels on both sides of every output:
    the threads of a partial tile (or block) that lie outside the image store nothing, and every pixel inside it is written."""
    import ctypes as C
    from v3d_amd.recon import mesh_refine as RFN
    kind, seed, W, H, _, cull, bits = case
    assert (W, H) in ((37, 21), (13, 9)) and (W % 16 and H % 16)
    cam = M.case_camera(case)
    v, f, c = M.mesh_scene(kind, seed)
    gc = gs_camera(cam, BG)
    zv, _, pix_q = MR.project_vertices(gc, v.to(DEV), bits)
    faces, colors = f.to(DEV, torch.int32).contiguous(), c.to(DEV).contiguous()
    ranges, vals_s, zmin = binned(gc, faces, pix_q, zv, cull, bits)
    lib = G.load_library()
    HW = H * W
    for count_hits in (True, False):
        want = MR.render_mesh(cam, v, f, c, BG, cull=cull, count_hits=count_hits, subpixel_bits=bits)
        bufs = {"render": guarded(3 * HW, torch.float32), "depth": guarded(HW, torch.float32), "alpha": guarded(HW, torch.float32),
                "face_id": guarded(HW, torch.int32), "n_hit": guarded(HW, torch.int32)}
        assert lib.v3d_recon_mesh_render(ranges.data_ptr(), vals_s.data_ptr(), faces.data_ptr(), faces.shape[0], pix_q.data_ptr(), zv.data_ptr(),
                                         zmin.data_ptr(), colors.data_ptr(), C.byref(gc), bits, bufs["render"][1], bufs["depth"][1], bufs["alpha"][1],
                                         bufs["face_id"][1], bufs["n_hit"][1] if count_hits else None, None) == 0
        torch.cuda.synchronize()
        for k, (buf, _) in bufs.items():
            if k == "n_hit" and not count_hits:
                assert bool((buf[GUARD:GUARD + HW] == PREFILL[torch.int32]).all()) and bool((buf[:GUARD] == SENTINEL[torch.int32]).all())
                continue
            body = assert_guards_untouched(buf, 3 * HW if k == "render" else HW, k)
            assert torch.equal(body, want[k].cpu().reshape(-1)), f"{k} differs from render_mesh"
    face_id = want["face_id"].contiguous()
    pv, pw = guarded(3 * HW, torch.int32), guarded(3 * HW, torch.float32)
    assert lib.v3d_recon_mesh_pixel_weights(face_id.data_ptr(), faces.data_ptr(), faces.shape[0], pix_q.data_ptr(), zv.data_ptr(), zv.shape[0], W, H, bits,
                                            pv[1], pw[1], None) == 0
    torch.cuda.synchronize()
    got_v, got_w = assert_guards_untouched(pv[0], 3 * HW, "pix_vert"), assert_guards_untouched(pw[0], 3 * HW, "pix_w")
    want_v, want_w = RFN.pixel_weights(face_id, faces, pix_q, zv, bits)
    assert torch.equal(got_v, want_v.cpu().reshape(-1)) and torch.equal(got_w, want_w.cpu().reshape(-1))
    assert int((got_v >= 0).sum()) == 3 * int((face_id >= 0).sum()) > 0


# ---- 10. the early exit where it must not fire, and a tie across batches --------------------------------------------------------------
def bars(out, ref, ref32, name, extra=None):
    derr, ierr = float((out["depth"].double() - ref["depth"]).abs().max()), float((out["render"].double() - ref["image"]).abs().max())
    derr32, ierr32 = float((ref32["depth"].double() - ref["depth"]).abs().max()), float((ref32["image"].double() - ref["image"]).abs().max())
    print(f"depth {derr:.3e} (float32 restatement {derr32:.3e})  image {ierr:.3e} ({ierr32:.3e})")
    record_parity(name, {"depth_max_abs": derr, "depth_float32_restatement": derr32, "image_max_abs": ierr, "image_float32_restatement": ierr32,
                         **(extra or {})})
    assert derr <= 4 * derr32 and ierr <= 4 * ierr32


def counted_and_fast(W, H, q, zv, faces, colors, cull=False, bits=8):
    counted, fast = raster(W, H, q, zv, faces, colors, cull, True, bits=bits), raster(W, H, q, zv, faces, colors, cull, False, bits=bits)
    assert "n_hit" not in fast
    for k in ("face_id", "depth", "render", "alpha"):
        assert torch.equal(counted[k], fast[k]), f"{k} differs between the counted walk and the early exit"
    return counted, fast


def test_early_exit_does_not_fire_while_a_later_batch_can_still_win():
    W, H = 56, 40
    q, zv, faces, colors = M.steep_cover(seed=M.SYNTH_SEEDS["steep_cover"])
    ref = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False)
    ref32 = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False, dtype=torch.float32)
    counted, fast = counted_and_fast(W, H, q, zv, faces, colors)
    r = counted["ranges"]
    assert int(r[0, 1] - r[0, 0]) == faces.shape[0] > 2 * 256          # tile 0: 3 batches, the layers in the last
    assert_same_decisions(counted, ref)
    assert_same_decisions(fast, ref, n_hit=False)
    first_layer = 1 + M.STEEP_FILLERS
    assert int((fast["face_id"][:16, :16] == first_layer).sum()) > 50  # the layer of the third batch wins where face 0 is deeper
    bars(counted, ref, ref32, "mesh_render_steep_cover")


@pytest.mark.parametrize("count_hits", (False, True), ids=("early-exit", "counted"))
def test_lower_face_index_wins_a_tie_across_a_batch_boundary(count_hits):
    W, H = 56, 40
    x, y = M.TIE_PIXEL
    q, zv, faces, colors = M.tie_across_batches(seed=M.SYNTH_SEEDS["tie_across_batches"])
    ref = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False)
    out = raster(W, H, q, zv, faces, colors, False, count_hits)
    r = out["ranges"]
    assert int(r[0, 1] - r[0, 0]) == faces.shape[0] == 2 * 256 + 1      # face 0 is the first entry of the third batch
    assert int(out["face_id"][y, x]) == 0 and float(out["depth"][y, x]) == 2.0
    assert float((out["render"][:, y, x] - colors[0]).abs().max()) <= 1e-6      # face 0's colour, not face 1's
    assert float((colors[0] - colors[3]).abs().max()) > 0.1
    assert_same_decisions(out, ref, n_hit=count_hits)
    if count_hits:
        assert int(out["n_hit"][y, x]) == 2
        bars(out, ref, M.rasterize(q, zv, faces, colors, W, H, BG, cull=False, dtype=torch.float32), "mesh_render_tie_across_batches")


# ---- 11. extreme coordinates, the image limit, absent faces ---------------------------------------------------------------------------
def test_corners_at_the_coordinate_limit():
    W, H = 56, 40
    q, zv, faces, colors = M.limit_triangle()
    ref = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False)
    ref32 = M.rasterize(q, zv, faces, colors, W, H, BG, cull=False, dtype=torch.float32)
    counted, fast = counted_and_fast(W, H, q, zv, faces, colors)
    assert counted["tiles_touched"].tolist() == [12, 9] and counted["n_inst"] == 21
    assert_same_decisions(counted, ref)
    assert bool((counted["n_hit"] >= 1).all()) and bool((counted["alpha"] == 1).all())
    bars(counted, ref, ref32, "mesh_render_limit_triangle")
    culled = raster(W, H, q, zv, faces.flip(1), colors, True, True)       # the other winding, culled: the same coverage or none at all
    ref_c = M.rasterize(q, zv, faces.flip(1), colors, W, H, BG, cull=True)
    assert_same_decisions(culled, ref_c)


@pytest.mark.parametrize("cull", (True, False), ids=("cull", "nocull"))
@pytest.mark.parametrize("size", M.LIMIT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_images_at_the_size_limit(size, cull):
    W, H = size
    cam = D.cams_for(W, H)[M.LIMIT_VIEW]
    v, f, c = M.mesh_scene("pair", M.LIMIT_SEEDS[size])
    zv, _, pix_q = (t.cpu() for t in MR.project_vertices(gs_camera(cam, BG), v.to(DEV)))
    q, zz, faces, colors = M.with_extra(pix_q, zv, f, c, M.limit_extra(W, H))
    ref = M.rasterize(q, zz, faces, colors, W, H, BG, cull=cull)
    ref32 = M.rasterize(q, zz, faces, colors, W, H, BG, cull=cull, dtype=torch.float32)
    assert float(ref["gap"].min()) >= M.Z_GAP_MARGIN                     # the CPU test's margin, on the kernel's own snap
    counted, fast = counted_and_fast(W, H, q, zz, faces, colors, cull)
    assert_same_decisions(counted, ref)
    last = counted["face_id"][:, -1] if W > H else counted["face_id"][-1, :]
    assert bool((last == f.shape[0]).any()) and int(counted["face_id"][0, 0]) == f.shape[0] + 1
    assert int(counted["tiles_touched"][-1]) == 256 and torch.equal(counted["tiles_touched"].long().cpu(), ref["tiles"])
    bars(counted, ref, ref32, f"mesh_render_image_limit[{W}x{H}-{'cull' if cull else 'nocull'}]", {"covered": float(ref["alpha"].mean())})


def test_faces_with_indices_outside_the_vertex_array_are_absent():
    from v3d_amd.recon import mesh_refine as RFN
    W, H = 37, 21
    cam = D.cams_for(W, H)[1]
    v, f, c = M.mesh_scene("sphere", M.SEEDS["sphere"])
    V = v.shape[0]
    gc = gs_camera(cam, BG)
    zv, _, pix_q = MR.project_vertices(gc, v.to(DEV))
    absent = torch.tensor([[-1, 0, 1], [0, V, 1], [0, 1, 2 ** 31 - 1], [-(2 ** 31), 1, 2], [V + 7, V, -1]], dtype=torch.long)
    both = torch.cat([f, absent]).to(DEV, torch.int32).contiguous()
    alone = f.to(DEV, torch.int32).contiguous()
    for cull in (True, False):
        for count_hits in (True, False):
            a = MR.rasterize_projected(gc, alone, pix_q, zv, c.to(DEV), cull, count_hits)
            b = MR.rasterize_projected(gc, both, pix_q, zv, c.to(DEV), cull, count_hits)
            assert float(a["alpha"].mean()) > 0.1
            for k in ("render", "depth", "alpha", "face_id") + (("n_hit",) if count_hits else ()):
                assert torch.equal(a[k], b[k]), f"{k} changes beside absent faces"
            assert not b["tiles_touched"][f.shape[0]:].any() and torch.equal(b["tiles_touched"][:f.shape[0]], a["tiles_touched"])
            assert b["n_inst"] == a["n_inst"] and torch.equal(a["ranges"], b["ranges"])
        va, vb = RFN.freeze_projected(gc, alone, pix_q, zv, BG, cull), RFN.freeze_projected(gc, both, pix_q, zv, BG, cull)
        assert torch.equal(va.pix_vert, vb.pix_vert) and torch.equal(va.pix_w, vb.pix_w) and torch.equal(va.ent_pix, vb.ent_pix)
    only = MR.rasterize_projected(gc, absent.to(DEV, torch.int32).contiguous(), pix_q, zv, c.to(DEV), False, True)      # nothing but absent faces
    assert only["n_inst"] == 0 and not only["tiles_touched"].any()
    assert_empty(only, H, W)
