"""Geometry from the splats on the gfx950 kernels of libv3d_recon.so (csrc_recon/geom.hip, v3d_amd/recon/geometry.py) against the torch
restatement (tests/recon_geom_ref.py): depth and alpha maps, TSDF integration, surface nets on an exact sphere (closed, oriented, the right
size), partial observation, the empty volume, and Gaussians -> mesh end to end.  The decision margins of the scenes are held on the CPU
(tests/test_recon_geom_cpu.py)."""
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
    W, H = 56, 40
    scene, cam = R.depth_case(("random", D.SCENE_SEEDS[0], W, H, 0))
    g = model(scene)
    _, st = RZ.forward_pass(hip_ops, g.xyz, g.scaling, g.rotation, g.opacity, g.features_dc, RZ.gs_camera(cam, [0, 0, 0]))
    lib = G.load_library()
    pad = 64 * 48 - W * H          # the tiles cover 64 x 48 pixels
    bufs = [torch.full((W * H + pad,), -7.0, device=DEV) for _ in range(2)]
    rc = lib.v3d_recon_depth_alpha(st["ranges"].data_ptr(), st["vals_s"].data_ptr(), st["means2d"].data_ptr(), st["conic_opacity"].data_ptr(),
                                   st["depth"].data_ptr(), st["n_contrib"].data_ptr(), W, H, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.v3d_recon_last_error()
    depth, alpha = G.depth_alpha(st, W, H)
    for b, m in zip(bufs, (depth, alpha)):
        assert torch.equal(b[:W * H].view(H, W), m) and bool((b[W * H:] == -7.0).all())


def test_no_gaussians_give_the_background_and_empty_maps():
    cam = D.cams_for(56, 40)[0]
    none = types.SimpleNamespace(xyz=torch.zeros(0, 3, device=DEV), scaling=torch.zeros(0, 3, device=DEV), rotation=torch.zeros(0, 4, device=DEV),
                                 opacity=torch.zeros(0, 1, device=DEV), features_dc=torch.zeros(0, 1, 3, device=DEV))
    out = G.render_geometry(cam, none, [0.25, 0.5, 1.0])
    assert out["render"].shape == (3, 40, 56) and torch.equal(out["render"][:, 3, 5].cpu(), torch.tensor([0.25, 0.5, 1.0]))
    assert out["depth"].shape == (40, 56) and not out["depth"].any() and not out["alpha"].any() and out["radii"].numel() == 0


# ---- TSDF -----------------------------------------------------------------------------------------------------------------------------
def test_tsdf_matches_the_restatement():
    case = R.sphere_tsdf_case()
    ref, near = R.sphere_tsdf_restatement(case)
    assert float(near.double().mean()) <= R.MAX_EXCLUDED
    N = case["N"]

    def run():
        vol = G.new_volume(N, case["bound"])
        for cam, (d, a, img) in zip(case["cams"], case["maps"]):
            G.integrate_view(vol, d.to(DEV), a.to(DEV), img.to(DEV), cam)
        return vol

    vol, again = run(), run()
    assert vol.trunc == pytest.approx(ref["trunc"])
    for k in ("tsdf_sum", "weight", "rgb_sum", "rgb_weight"):
        assert torch.equal(getattr(vol, k), getattr(again, k)), f"{k} differs between two runs"
    keep = ~near
    w = vol.weight.cpu().double().reshape(-1)
    assert torch.equal(w[keep], ref["weight"][keep])
    assert torch.equal(vol.rgb_weight.cpu().double().reshape(-1)[keep], ref["rgb_weight"][keep])
    mean = vol.tsdf_sum.cpu().double().reshape(-1) / w.clamp_min(1)
    err = float((mean - ref["tsdf_sum"] / ref["weight"].clamp_min(1))[keep].abs().max())
    rgb_err = float((vol.rgb_sum.cpu().double().reshape(3, -1) - ref["rgb_sum"])[:, keep].abs().max())
    print(f"mean TSDF {err:.3e}  rgb_sum {rgb_err:.3e}  excluded {float(near.double().mean()):.3%}  differing weights among the excluded: "
          f"{int((w != ref['weight'])[near].sum())}")
    record_parity("recon_geom_tsdf", {"mean_tsdf_max_abs": err, "rgb_sum_max_abs": rgb_err, "excluded_share": float(near.double().mean())})
    assert err <= 1e-5
    assert rgb_err <= 1e-5          # sums of at most 4 colours in 0 .. 1 that both sides read from the same float32 image


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
