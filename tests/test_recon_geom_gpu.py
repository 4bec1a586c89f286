"""Geometry from the splats on the gfx950 kernels of libv3d_recon.so (csrc_recon/geom.hip, v3d_amd/recon/geometry.py) against the torch
restatement (tests/recon_geom_ref.py): depth and alpha maps, TSDF integration, surface nets on an exact sphere (closed, oriented, the right
size), partial observation, the empty volume, and Gaussians -> mesh end to end.  Beside the shapes the kernels were written at: portrait
images and one narrower than a tile, volumes whose launches end in a partial block (with guard elements behind every output), views
that are not square, cameras inside the volume, random volumes that take nearly every corner-sign configuration of a cell, and planes that
leave through the volume's border or pass through voxels whose mean is exactly 0.  The decision margins of the scenes and what each volume
covers are held on the CPU (tests/test_recon_geom_cpu.py)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import recon_geom_ref as R
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import rasterize as RZ

pytestmark = pytest.mark.gpu
DEV = "cuda"


def model(scene):
    xyz, scale, rot, op, fdc = (t.to(DEV) for t in scene)
    return types.SimpleNamespace(xyz=xyz, scaling=scale, rotation=rot, opacity=op, features_dc=fdc.view(-1, 1, 3).contiguous())


def device_volume(ref):
    """A TsdfVolume on the GPU holding a restatement volume's state (float32)"""
    N = ref["N"]
    f = lambda t, *s: t.float().reshape(*s).contiguous().to(DEV)  # noqa: E731
    return G.TsdfVolume(N, ref["bound"], ref["trunc"], f(ref["tsdf_sum"], N, N, N), f(ref["weight"], N, N, N), f(ref["rgb_sum"], 3, N, N, N),
                        f(ref["rgb_weight"], N, N, N))


# ---- depth / alpha --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DEPTH_CASES, ids=R.depth_case_id)
def test_depth_and_alpha_match_the_fp64_oracle(hip_ops, case):
    _, _, W, H, _ = case
    scene, cam = R.depth_case(case)
    bg = [1.0, 1.0, 1.0]
    ref = R.depth_alpha(scene, cam, W, H)
    g = model(scene)
    out = G.render_geometry(cam, g, bg)
    again = G.render_geometry(cam, g, bg)
    assert set(out) == {"render", "depth", "alpha", "radii"} and out["depth"].shape == (H, W) and out["alpha"].shape == (H, W)
    for k in ("render", "depth", "alpha"):
        assert torch.equal(out[k], again[k]), f"{k} differs between two runs"
    # `final_T` is the colour pass's own output (rasterize.forward_pass): the maps end at its last contributor, so alpha restates 1 - final_T.
    # Against the fp64 oracle's transmittance the float32 run of the restatement is itself off by 0.9e-6 .. 2.0e-6 on these cases (the number
    # format: a product of dozens of fp32 factors), so that comparison is held at the colour bar like the image.
    _, st = RZ.forward_pass(hip_ops, g.xyz, g.scaling, g.rotation, g.opacity, g.features_dc, RZ.gs_camera(cam, bg))
    alpha_err = float((out["alpha"].double() - (1 - st["final_T"].double())).abs().max())
    alpha_oracle_err = float((out["alpha"].double().cpu() - (1 - ref["final_T"])).abs().max())
    depth_err = float((out["depth"].double().cpu() - ref["depth"]).abs().max())
    img_err = float((out["render"].double().cpu() - R.image_of(ref, bg, W, H)).abs().max())
    zmax = ref["zmax"]
    print(f"alpha vs 1 - final_T {alpha_err:.3e}, vs fp64 oracle {alpha_oracle_err:.3e}  depth {depth_err:.3e} (z <= {zmax:.3f}: "
          f"{depth_err / zmax:.3e} relative)  image {img_err:.3e}")
    record_parity(f"recon_geom_depth_alpha[{R.depth_case_id(case)}]", {"alpha_vs_final_T_max_abs": alpha_err, "alpha_vs_fp64_oracle_max_abs": alpha_oracle_err,
                                                                        "depth_max_abs": depth_err, "zmax": zmax, "depth_over_zmax": depth_err / zmax})
    assert torch.equal(st["n_contrib"].cpu(), ref["n_contrib"])        # the same last contributor as the oracle's colour image
    assert alpha_err <= 1e-6
    assert alpha_oracle_err <= 1e-4
    assert depth_err <= 1e-4 * zmax         # the colour bar of DESIGN.md 3.7, on values scaled by view z instead of by a unit colour
    assert img_err <= 1e-4                  # (the colour image beside the maps is the rasterizer's)
    assert float(out["alpha"].max()) > 0.5 and float(out["depth"].max()) > 0.5      # (a scene, not an empty view)


def test_depth_pass_writes_no_pixel_outside_a_ragged_image(hip_ops):
    # landscape, portrait, and a single column of tiles; (tiles cover)
    for case, cover in ((("random", D.SCENE_SEEDS[0], 56, 40, 0), (64, 48)), (("random", 1116, 40, 56, 1), (48, 64)), (("random", 1116, 8, 24, 1), (16, 32))):
        W, H = case[2:4]
        scene, cam = R.depth_case(case)
        g = model(scene)
        _, st = RZ.forward_pass(hip_ops, g.xyz, g.scaling, g.rotation, g.opacity, g.features_dc, RZ.gs_camera(cam, [0, 0, 0]))
        lib = G.load_library()
        pad = cover[0] * cover[1] - W * H
        assert cover == (-(-W // 16) * 16, -(-H // 16) * 16) and pad > 0
        bufs = [torch.full((W * H + pad,), -7.0, device=DEV) for _ in range(2)]
        rc = lib.v3d_recon_depth_alpha(st["ranges"].data_ptr(), st["vals_s"].data_ptr(), st["means2d"].data_ptr(), st["conic_opacity"].data_ptr(),
                                       st["depth"].data_ptr(), st["n_contrib"].data_ptr(), W, H, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.v3d_recon_last_error()
        depth, alpha = G.depth_alpha(st, W, H)
        assert float(alpha.max()) > 0.5, "an empty view"
        for b, m in zip(bufs, (depth, alpha)):
            assert torch.equal(b[:W * H].view(H, W), m) and bool((b[W * H:] == -7.0).all()), (W, H)


def test_no_gaussians_give_the_background_and_empty_maps():
    cam = D.cams_for(56, 40)[0]
    none = types.SimpleNamespace(xyz=torch.zeros(0, 3, device=DEV), scaling=torch.zeros(0, 3, device=DEV), rotation=torch.zeros(0, 4, device=DEV),
                                 opacity=torch.zeros(0, 1, device=DEV), features_dc=torch.zeros(0, 1, 3, device=DEV))
    out = G.render_geometry(cam, none, [0.25, 0.5, 1.0])
    assert out["render"].shape == (3, 40, 56) and torch.equal(out["render"][:, 3, 5].cpu(), torch.tensor([0.25, 0.5, 1.0]))
    assert out["depth"].shape == (40, 56) and not out["depth"].any() and not out["alpha"].any() and out["radii"].numel() == 0


# ---- TSDF -----------------------------------------------------------------------------------------------------------------------------
def integrate_case(case):
    vol = G.new_volume(case["N"], case["bound"], case["trunc"])
    for cam, (d, a, img) in zip(case["cams"], case["maps"]):
        G.integrate_view(vol, d.to(DEV), a.to(DEV), img.to(DEV), cam, case["alpha_min"])
    return vol


@pytest.mark.parametrize("name", list(R.TSDF_CASES))
def test_tsdf_matches_the_restatement(name):
    case = R.sphere_tsdf_case(**R.TSDF_CASES[name])
    ref, near = R.sphere_tsdf_restatement(case)
    assert float(near.double().mean()) <= R.MAX_EXCLUDED
    vol, again = integrate_case(case), integrate_case(case)
    assert vol.trunc == pytest.approx(ref["trunc"])
    for k in ("tsdf_sum", "weight", "rgb_sum", "rgb_weight"):
        assert torch.equal(getattr(vol, k), getattr(again, k)), f"{k} differs between two runs"
    keep = ~near
    w = vol.weight.cpu().double().reshape(-1)
    mean = vol.tsdf_sum.cpu().double().reshape(-1) / w.clamp_min(1)
    err = float((mean - ref["tsdf_sum"] / ref["weight"].clamp_min(1))[keep].abs().max())
    rgb_err = float((vol.rgb_sum.cpu().double().reshape(3, -1) - ref["rgb_sum"])[:, keep].abs().max())
    print(f"mean TSDF {err:.3e}  rgb_sum {rgb_err:.3e}  excluded {float(near.double().mean()):.3%}  differing weights among the excluded: "
          f"{int((w != ref['weight'])[near].sum())}, among the others: {int((w != ref['weight'])[keep].sum())}")
    record_parity("recon_geom_tsdf" if name == "default" else f"recon_geom_tsdf[{name}]",
                  {"mean_tsdf_max_abs": err, "rgb_sum_max_abs": rgb_err, "excluded_share": float(near.double().mean())})
    assert torch.equal(w[keep], ref["weight"][keep])
    assert torch.equal(vol.rgb_weight.cpu().double().reshape(-1)[keep], ref["rgb_weight"][keep])
    assert err <= 1e-5
    assert rgb_err <= 1e-5          # sums of at most 5 colours in 0 .. 1 that both sides read from the same float32 image


def test_tsdf_pass_writes_nothing_outside_a_ragged_volume():
    """26^3 voxels end 168 threads into the last block.  The accumulators are the leading parts of buffers one block longer; the voxel just
    past the volume lies inside one of the views (tests/test_recon_geom_cpu.py), so a thread let through there would write."""
    case = R.sphere_tsdf_case(**R.TSDF_CASES[R.TSDF_CANARY_CASE])
    N = case["N"]
    n3 = N ** 3
    assert n3 % 256 == 168
    lib = G.load_library()
    bufs = [torch.full((k * n3 + 256,), -7.0, device=DEV) for k in (1, 1, 3, 1)]       # tsdf_sum, weight, rgb_sum, rgb_weight
    for b in bufs:
        b[:-256] = 0
    for cam, (d, a, img) in zip(case["cams"], case["maps"]):
        d, a, img = d.to(DEV), a.to(DEV), img.to(DEV)
        gc = RZ.gs_camera(cam, [0.0, 0.0, 0.0])
        rc = lib.v3d_recon_tsdf_integrate(d.data_ptr(), a.data_ptr(), img.data_ptr(), C.byref(gc), N, case["bound"], case["trunc"], case["alpha_min"],
                                          *(b.data_ptr() for b in bufs), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.v3d_recon_last_error()
    vol = integrate_case(case)
    assert float(vol.weight.max()) == len(case["cams"]) and float(vol.rgb_weight.max()) > 0
    for b, m in zip(bufs, (vol.tsdf_sum, vol.weight, vol.rgb_sum, vol.rgb_weight)):
        assert torch.equal(b[:-256], m.reshape(-1)), "the leading part is not what integrate_view accumulates"
        assert bool((b[-256:] == -7.0).all()), "a guard element behind the volume was written"


def test_integrate_view_refuses_transposed_maps():
    cam = D.cams_for(40, 24)[0]
    vol = G.new_volume(8, 1.0)
    t = lambda *shape: torch.zeros(*shape, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="do not match the 40 x 24 camera"):
        G.integrate_view(vol, t(40, 24), t(40, 24), t(3, 40, 24), cam)
    with pytest.raises(ValueError, match="do not match the 40 x 24 camera"):
        G.integrate_view(vol, t(24, 40), t(24, 40), t(3, 40, 24), cam)
    G.integrate_view(vol, t(24, 40), t(24, 40), t(3, 24, 40), cam)
    assert not vol.rgb_weight.any()


# ---- surface nets ---------------------------------------------------------------------------------------------------------------------
SPHERE = dict(N=24, bound=1.0, radius=0.5)


@pytest.fixture(scope="module")
def sphere():
    ref = R.sphere_volume(SPHERE["N"], SPHERE["bound"], SPHERE["radius"])
    verts, faces, colors = G.extract_mesh(device_volume(ref))
    return ref, verts.cpu(), faces.cpu(), colors.cpu()


def test_sphere_mesh_is_closed_oriented_and_the_right_size(sphere):
    _, verts, faces, colors = sphere
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and colors.dtype == torch.float32
    assert verts.shape[1] == 3 and faces.shape[1] == 3 and colors.shape == verts.shape and faces.shape[0] > 100
    assert int(faces.min()) == 0 and int(faces.max()) == verts.shape[0] - 1
    und, cnt, dirsum = R.undirected_counts(faces.numpy())
    assert (cnt == 2).all(), "an edge does not lie in exactly two triangles"
    assert (dirsum == 0).all(), "two triangles run a shared edge in the same direction"
    assert verts.shape[0] - und.shape[0] + faces.shape[0] == 2
    voxel, r = 2 * SPHERE["bound"] / SPHERE["N"], SPHERE["radius"]
    assert float((verts.double().norm(dim=1) - r).abs().max()) <= voxel
    vol = R.signed_volume(verts.numpy(), faces.numpy())
    assert 4 / 3 * np.pi * (r - voxel) ** 3 < vol < 4 / 3 * np.pi * (r + voxel) ** 3, vol


def test_sphere_mesh_is_the_restatements(sphere):
    ref, verts, faces, colors = sphere
    rv, rf, rc, _, _ = R.extract({k: (v.double() if torch.is_tensor(v) else v) for k, v in ref.items()})
    assert verts.shape == rv.shape and torch.equal(faces.long(), rf)            # same cells, same edges, same order, same winding
    # a vertex is a mean of up to 12 quotients of float32 means in 0 .. 1, scaled by a voxel of 0.083: a few ulp of 1
    assert float((verts.double() - rv).abs().max()) <= 1e-6
    assert float((colors.double() - rc).abs().max()) <= 1e-6
    again = G.extract_mesh(device_volume(ref))
    assert torch.equal(again[0].cpu(), verts) and torch.equal(again[1].cpu(), faces) and torch.equal(again[2].cpu(), colors)


def test_unobserved_octant_leaves_the_mesh_open():
    ref = R.sphere_volume(SPHERE["N"], SPHERE["bound"], SPHERE["radius"])
    N, h = SPHERE["N"], SPHERE["N"] // 2
    w = ref["weight"].reshape(N, N, N).clone()
    w[h:, h:, h:] = 0
    ref["weight"] = w.reshape(-1)
    verts, faces, _ = (t.cpu() for t in G.extract_mesh(device_volume(ref)))
    assert faces.shape[0] > 100
    voxel = 2 * SPHERE["bound"] / N
    cell = torch.floor((verts.double() + SPHERE["bound"]) / voxel - 0.5).long()          # the cell (lower corner voxel) a vertex lies in
    assert int(cell.min()) >= 0 and int(cell.max()) <= N - 2
    used = torch.zeros(verts.shape[0], dtype=torch.bool)
    used[faces.long().reshape(-1)] = True
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                seen = w[cell[:, 2] + dz, cell[:, 1] + dy, cell[:, 0] + dx] > 0
                assert bool(seen.all()), "a vertex sits in a cell with an unobserved corner"
    assert not bool((cell >= h).all(1).any())                                             # nothing inside the unobserved octant
    _, cnt, _ = R.undirected_counts(faces.numpy())
    assert (cnt <= 2).all() and int((cnt == 1).sum()) > 0, "the mesh should be open along the unobserved octant"
    rv, rf, _, _, _ = R.extract({k: (v.double() if torch.is_tensor(v) else v) for k, v in ref.items()})
    assert torch.equal(faces.long(), rf) and float((verts.double() - rv).abs().max()) <= 1e-6
    assert bool(used.any())


def test_empty_volume_gives_empty_arrays():
    vol = G.new_volume(24, 1.0)
    vol.tsdf_sum.fill_(1.0)
    vol.weight.fill_(1.0)
    verts, faces, colors = G.extract_mesh(vol)
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and colors.shape == (0, 3)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32
    verts, faces, colors = G.extract_mesh(G.new_volume(24, 1.0))          # nothing observed at all
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and colors.shape == (0, 3)


@pytest.mark.parametrize("name", list(R.MESH_VOLUMES))
def test_mesh_of_a_random_or_plane_volume_is_the_restatements(name):
    """Every decision of the extraction is the sign of a numerator or a weight against 0, so the kernels and the fp64 restatement of the same
    float32 values must agree on every cell, edge, index and winding; positions and colours are a few ulp of 1 apart."""
    ref = R.MESH_VOLUMES[name]()
    verts, faces, colors = (t.cpu() for t in G.extract_mesh(device_volume(ref)))
    rv, rf, rc, _, _ = R.extract(R.promoted(ref))
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and colors.dtype == torch.float32
    assert verts.shape == rv.shape and colors.shape == rc.shape and faces.shape == rf.shape and faces.shape[1] == 3
    assert torch.equal(faces.long(), rf)
    vert_err, col_err = float((verts.double() - rv).abs().max()), float((colors.double() - rc).abs().max())
    grey = (rc == 0.5).all(1)          # a random volume's vertices with no coloured corner (a plane's colours are means that may land on 0.5)
    print(f"{verts.shape[0]} vertices ({int(grey.sum())} grey), {faces.shape[0]} triangles; vertices {vert_err:.3e}  colours {col_err:.3e}")
    record_parity(f"recon_geom_mesh[{name}]", {"vertices": int(verts.shape[0]), "triangles": int(faces.shape[0]), "grey_vertices": int(grey.sum()),
                                               "vertex_max_abs": vert_err, "colour_max_abs": col_err})
    assert vert_err <= 1e-6
    assert col_err <= 1e-6
    assert not name.startswith("random") or bool((colors[grey] == 0.5).all())
    again = G.extract_mesh(device_volume(ref))
    assert torch.equal(again[0].cpu(), verts) and torch.equal(again[1].cpu(), faces) and torch.equal(again[2].cpu(), colors)


def test_one_cell_gives_a_vertex_and_no_faces():
    verts, faces, colors = G.extract_mesh(device_volume(R.MESH_VOLUMES["random2"]()))
    assert verts.shape == (1, 3) and colors.shape == (1, 3) and faces.shape == (0, 3) and faces.dtype == torch.int32


def test_extraction_writes_nothing_outside_its_outputs(hip_ops):
    """random_volume(13, 2): 12^3 cells and 3 * 13^3 edges both end in a partial block.  The five entries in extract_mesh's order, every
    output the leading part of a buffer 256 elements longer."""
    ref = R.MESH_VOLUMES["random13"]()
    vol = device_volume(ref)
    N = vol.resolution
    m3, e3 = (N - 1) ** 3, 3 * N ** 3
    assert m3 % 256 and e3 % 256 and N ** 3 % 256
    lib, st = G.load_library(), torch.cuda.current_stream().cuda_stream
    ts, w, rs, rw = (t.data_ptr() for t in (vol.tsdf_sum, vol.weight, vol.rgb_sum, vol.rgb_weight))
    guarded = lambda n, dtype: torch.full((n + 256,), -7, dtype=dtype, device=DEV)  # noqa: E731
    cflags = guarded(m3, torch.int32)
    assert lib.v3d_recon_cells_flag(ts, w, N, cflags.data_ptr(), st) == 0, lib.v3d_recon_last_error()
    coffs = hip_ops.gs_scan(cflags[:m3])
    nv = int(coffs[-1])
    verts, colors = guarded(3 * nv, torch.float32), guarded(3 * nv, torch.float32)
    assert lib.v3d_recon_cells_vertices(ts, w, rs, rw, N, vol.bound, cflags.data_ptr(), coffs.data_ptr(), verts.data_ptr(), colors.data_ptr(), st) == 0, \
        lib.v3d_recon_last_error()
    eflags = guarded(e3, torch.int32)
    assert lib.v3d_recon_edges_flag(ts, w, N, cflags.data_ptr(), eflags.data_ptr(), st) == 0, lib.v3d_recon_last_error()
    eoffs = hip_ops.gs_scan(eflags[:e3])
    ne = int(eoffs[-1])
    faces = guarded(6 * ne, torch.int32)
    assert lib.v3d_recon_edges_faces(ts, w, N, coffs.data_ptr(), eflags.data_ptr(), eoffs.data_ptr(), faces.data_ptr(), st) == 0, lib.v3d_recon_last_error()
    ev, ef, ec = G.extract_mesh(vol)
    assert (nv, 2 * ne) == (ev.shape[0], ef.shape[0]) and nv > 1000 and ne > 1000
    for buf, n, out in ((verts, 3 * nv, ev), (colors, 3 * nv, ec), (faces, 6 * ne, ef)):
        assert torch.equal(buf[:n], out.reshape(-1)), "the leading part is not what extract_mesh returns"
    _, _, _, rflags, _ = R.extract(R.promoted(ref))
    assert torch.equal(cflags[:m3].cpu().bool(), rflags) and int(eflags[:e3].sum()) == ne and bool(((eflags[:e3] == 0) | (eflags[:e3] == 1)).all())
    for buf in (cflags, eflags, verts, colors, faces):
        assert bool((buf[-256:] == -7).all()), "a guard element behind an output was written"


def test_extract_mesh_refuses_other_types_and_devices():
    ref = R.MESH_VOLUMES["random3"]()
    vol = device_volume(ref)
    vol.tsdf_sum = vol.tsdf_sum.double()
    with pytest.raises(RuntimeError, match=r"tsdf_sum: expected a float32 tensor in device memory, got torch.float64 on cuda:0"):
        G.extract_mesh(vol)
    vol = device_volume(ref)
    vol.rgb_weight = vol.rgb_weight.cpu()
    with pytest.raises(RuntimeError, match=r"rgb_weight: expected a float32 tensor in device memory, got torch.float32 on cpu"):
        G.extract_mesh(vol)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_gaussians_to_mesh_end_to_end(tmp_path):
    """fuse_tsdf + extract_mesh on the kernels against the same views through the fp64 restatement (fp64-oracle depth and alpha).
    Bar: symmetric Chamfer distance of the two vertex sets <= 4 x what the float32 run of the restatement loses against its fp64 run
    (R.E2E_CHAMFER_FP32, measured on the CPU; measured again here on the device and recorded beside the kernels' figure)."""
    g = model(R.shell_scene())
    vol = G.fuse_tsdf(g, R.e2e_cameras(), resolution=R.E2E["N"], bound=R.E2E_BOUND, bg=[1.0, 1.0, 1.0])
    verts, faces, colors = G.extract_mesh(vol)
    ref64 = R.e2e_restatement(torch.float64, device=DEV)
    ref32 = R.e2e_restatement(torch.float32, device=DEV)
    cd32 = R.chamfer(ref32[0], ref64[0])
    cd = R.chamfer(verts.cpu(), ref64[0])
    print(f"Chamfer: kernels vs fp64 {cd:.3e}; float32 restatement vs fp64 {cd32:.3e} (on the CPU: {R.E2E_CHAMFER_FP32:.3e}); "
          f"vertices {verts.shape[0]} vs {ref64[0].shape[0]}, triangles {faces.shape[0]} vs {ref64[1].shape[0]}")
    record_parity("recon_geom_end_to_end", {"chamfer_kernels_vs_fp64": cd, "chamfer_float32_restatement_vs_fp64": cd32,
                                            "chamfer_float32_restatement_vs_fp64_cpu": R.E2E_CHAMFER_FP32, "vertices": int(verts.shape[0]),
                                            "vertices_fp64": int(ref64[0].shape[0]), "triangles": int(faces.shape[0])})
    path = str(tmp_path / "mesh.ply")
    G.save_mesh_ply(path, verts, faces, colors)
    v, f, c = G.read_mesh_ply(path)
    assert v.shape == tuple(verts.shape) and f.shape == tuple(faces.shape) and c.shape == tuple(colors.shape) and v.shape[0] > 1000
    assert 0.3 < float(np.linalg.norm(v, axis=1).mean()) < 0.6             # a shell about the sphere of radius 0.5
    assert cd <= 4 * R.E2E_CHAMFER_FP32


def test_gaussians_to_mesh_end_to_end_on_wide_views_and_a_ragged_volume():
    """The same scene on 72 x 40 views and 30^3 voxels (30^3 = 105 * 256 + 120), at the bar of test_gaussians_to_mesh_end_to_end:
    Chamfer(kernels, fp64 restatement) <= 4 x Chamfer(float32 restatement, fp64 restatement) as measured on the CPU
    (R.E2E_CHAMFER_FP32_RAGGED); measured again here on the device and recorded."""
    g = model(R.shell_scene())
    W, H, N = (R.E2E_RAGGED[k] for k in ("W", "H", "N"))
    assert N ** 3 % 256 == 120 and W != H
    vol = G.fuse_tsdf(g, R.e2e_cameras(W, H), resolution=N, bound=R.E2E_BOUND, bg=[1.0, 1.0, 1.0])
    verts, faces, colors = G.extract_mesh(vol)
    ref64 = R.e2e_restatement(torch.float64, device=DEV, **R.E2E_RAGGED)
    ref32 = R.e2e_restatement(torch.float32, device=DEV, **R.E2E_RAGGED)
    cd32 = R.chamfer(ref32[0], ref64[0])
    cd = R.chamfer(verts.cpu(), ref64[0])
    print(f"Chamfer: kernels vs fp64 {cd:.3e}; float32 restatement vs fp64 {cd32:.3e} (on the CPU: {R.E2E_CHAMFER_FP32_RAGGED:.3e}); "
          f"vertices {verts.shape[0]} vs {ref64[0].shape[0]}, triangles {faces.shape[0]} vs {ref64[1].shape[0]}")
    record_parity("recon_geom_end_to_end[72x40-n30]",
                  {"chamfer_kernels_vs_fp64": cd, "chamfer_float32_restatement_vs_fp64": cd32,
                   "chamfer_float32_restatement_vs_fp64_cpu": R.E2E_CHAMFER_FP32_RAGGED, "vertices": int(verts.shape[0]),
                   "vertices_fp64": int(ref64[0].shape[0]), "triangles": int(faces.shape[0])})
    assert verts.shape[0] > 1000 and colors.shape == verts.shape and 0 <= int(faces.min()) and int(faces.max()) < verts.shape[0]
    assert 0.3 < float(verts.norm(dim=1).mean()) < 0.6                       # a shell about the sphere of radius 0.5
    assert cd <= 4 * R.E2E_CHAMFER_FP32_RAGGED
