"""libv3d_recon.so (include/v3d_recon.h, v3d_amd/recon/geometry.py) without a GPU: the library builds, exports and binds every declared
symbol, refuses bad arguments before any launch, the mesh PLY round-trips, the new command-line flags parse, the torch restatement
(tests/recon_geom_ref.py) extracts a closed sphere, and the scenes of tests/test_recon_geom_gpu.py keep their decision margins."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import recon_geom_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    path = build_recon(verbose=False)
    assert os.path.exists(path)
    return geometry.load_library()


def test_library_builds_beside_the_kernel_library(lib):
    from v3d_amd import build
    assert os.path.basename(build.RECON_LIB) == "libv3d_recon.so" and os.path.dirname(build.RECON_LIB) == os.path.dirname(build.LIB)
    assert all(os.path.dirname(s) != build.CSRC for s in [os.path.join(build.RECON_CSRC, f) for f in os.listdir(build.RECON_CSRC)])
    assert lib.v3d_recon_abi_version() == 1


def test_header_symbols_are_exported_and_bound(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) >= 8, declared
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/v3d_recon.h but not exported"
    assert declared == set(geometry.SIGNATURES), (declared ^ set(geometry.SIGNATURES))
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION
    m = re.search(r"#define V3D_RECON_ABI_VERSION (\d+)", hdr)
    assert m and int(m.group(1)) == geometry.ABI_VERSION
    m = re.search(r"#define V3D_RECON_MAX_N (\d+)", hdr)
    assert m and int(m.group(1)) == geometry.MAX_RESOLUTION == 512


def _camera(W=32, H=32):
    from v3d_amd.recon.rasterize import gs_camera
    return gs_camera(D.cams_for(W, H)[0], [0, 0, 0])


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    cam = _camera()
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731
    assert lib.v3d_recon_depth_alpha(None, p, p, p, p, p, 32, 32, p, p, None) == -1 and "v3d_recon_depth_alpha" in err() and "null" in err()
    assert lib.v3d_recon_depth_alpha(p, p, p, p, p, p, 32, 32, None, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_depth_alpha(p, p, p, p, p, p, 0, 32, p, p, None) == -1 and "positive" in err()
    assert lib.v3d_recon_tsdf_integrate(p, p, p, None, 24, 1.0, 0.3, 0.5, p, p, p, p, None) == -1 and "v3d_recon_tsdf_integrate" in err()
    assert lib.v3d_recon_tsdf_integrate(p, None, p, C.byref(cam), 24, 1.0, 0.3, 0.5, p, p, p, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_tsdf_integrate(p, p, p, C.byref(cam), 513, 1.0, 0.3, 0.5, p, p, p, p, None) == -1 and "513" in err() and "512" in err()
    assert lib.v3d_recon_tsdf_integrate(p, p, p, C.byref(cam), 24, 0.0, 0.3, 0.5, p, p, p, p, None) == -1 and "positive" in err()
    assert lib.v3d_recon_tsdf_integrate(p, p, p, C.byref(cam), 24, 1.0, 0.0, 0.5, p, p, p, p, None) == -1 and "positive" in err()
    assert lib.v3d_recon_cells_flag(p, p, 513, p, None) == -1 and "512" in err()
    assert lib.v3d_recon_cells_flag(p, p, 1, p, None) == -1 and "v3d_recon_cells_flag" in err()
    assert lib.v3d_recon_cells_flag(p, None, 24, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_cells_vertices(p, p, p, p, 513, 1.0, p, p, p, p, None) == -1 and "512" in err()
    assert lib.v3d_recon_cells_vertices(p, p, p, p, 24, 1.0, p, p, None, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_edges_flag(p, p, 1024, p, p, None) == -1 and "512" in err()
    assert lib.v3d_recon_edges_flag(p, p, 24, None, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_edges_faces(p, p, 513, p, p, p, p, None) == -1 and "512" in err()
    assert lib.v3d_recon_edges_faces(p, p, 24, p, p, p, None, None) == -1 and "v3d_recon_edges_faces" in err()


def test_host_api_refuses_large_volumes_and_bad_maps():
    from v3d_amd.recon import geometry
    with pytest.raises(ValueError, match="512"):
        geometry.new_volume(513, 1.0, device="cpu")
    with pytest.raises(ValueError, match="positive"):
        geometry.new_volume(16, 0.0, device="cpu")
    vol = geometry.new_volume(16, 1.0, device="cpu")
    assert vol.trunc == pytest.approx(4 * 2.0 / 16) and vol.voxel == pytest.approx(0.125)
    assert vol.rgb_sum.shape == (3, 16, 16, 16) and vol.weight.shape == (16, 16, 16)


def test_mesh_ply_round_trip(tmp_path):
    from v3d_amd.recon import geometry
    rng = np.random.default_rng(0)
    verts = rng.standard_normal((50, 3)).astype(np.float32)
    faces = rng.integers(0, 50, size=(80, 3)).astype(np.int32)
    colors = rng.random((50, 3)).astype(np.float32)
    colors[0], colors[1] = (-0.5, 0.0, 2.0), (1.0, 0.5, 0.25)
    path = str(tmp_path / "sub" / "mesh.ply")
    geometry.save_mesh_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), colors)
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode().splitlines()
    assert head == ["ply", "format binary_little_endian 1.0", "element vertex 50", "property float x", "property float y", "property float z",
                    "property uchar red", "property uchar green", "property uchar blue", "element face 80",
                    "property list uchar int vertex_indices"]
    assert len(raw) == raw.index(b"end_header\n") + 11 + 50 * 15 + 80 * 13
    v, f, c = geometry.read_mesh_ply(path)
    np.testing.assert_array_equal(v, verts)
    np.testing.assert_array_equal(f, faces)
    np.testing.assert_array_equal(c, np.rint(np.clip(colors, 0, 1) * 255).astype(np.uint8))
    assert tuple(c[0]) == (0, 0, 255) and tuple(c[1]) == (255, 128, 64)
    empty = str(tmp_path / "empty.ply")
    geometry.save_mesh_ply(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    v, f, c = geometry.read_mesh_ply(empty)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        geometry.save_mesh_ply(empty, verts, faces + 50, colors)


def _entry():
    spec = importlib.util.spec_from_file_location("v3d_recon_entry_geom", os.path.join(ROOT, "scripts", "pub", "recon_from_vid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mesh_flags_parse_and_are_off_by_default():
    ap = _entry().build_parser()
    base = ["-w", "--sh_degree", "0", "--iterations", "4000", "--lambda_dssim", "1.0", "--lambda_lpips", "0", "--save_iterations", "4000",
            "--num_pts", "100000", "--video", "x.npy", "-m", "out/gs", "--render_orbit", "36"]
    a = vars(ap.parse_args(base))
    assert a["save_mesh"] is None and a["render_depth"] == 0 and a["mesh_resolution"] == 256
    old = {"white_background": True, "sh_degree": 0, "iterations": 4000, "lambda_dssim": 1.0, "lambda_lpips": 0.0, "save_iterations": [4000],
           "num_pts": 100000, "num_frames": None, "radius": 2.0, "elevation": 0.0, "fov": 60.0, "seed": 0, "model_path": "out/gs", "video": "x.npy",
           "input_path": None, "synthetic": False, "checkpoint_path": None, "num_steps": None, "render_orbit": 36}
    assert {k: v for k, v in a.items() if k not in ("save_mesh", "mesh_resolution", "render_depth")} == old
    b = vars(ap.parse_args(base + ["--save_mesh", "--mesh_resolution", "128", "--render_depth", "12"]))
    assert b["save_mesh"] == "" and b["mesh_resolution"] == 128 and b["render_depth"] == 12        # "" -> <model_path>/mesh.ply
    assert {k: v for k, v in b.items() if k not in ("save_mesh", "mesh_resolution", "render_depth")} == old
    assert ap.parse_args(base + ["--save_mesh", "m.ply"]).save_mesh == "m.ply"


def test_restatement_extracts_a_closed_sphere():
    N, bound, r = 24, 1.0, 0.5
    verts, faces, colors, flags, _ = R.extract(R.sphere_volume(N, bound, r, torch.float64))
    und, cnt, dirsum = R.undirected_counts(faces.numpy())
    assert (cnt == 2).all() and (dirsum == 0).all()
    assert verts.shape[0] - und.shape[0] + faces.shape[0] == 2
    voxel = 2 * bound / N
    assert float((verts.norm(dim=1) - r).abs().max()) <= voxel
    vol = R.signed_volume(verts.numpy(), faces.numpy())
    assert 4 / 3 * np.pi * (r - voxel) ** 3 < vol < 4 / 3 * np.pi * (r + voxel) ** 3
    assert int(flags.sum()) == verts.shape[0] and float(colors.min()) >= 0 and float(colors.max()) <= 1


def test_depth_scenes_keep_their_margin():
    # depth and alpha are held to the fp64 oracle at a continuous bar: every alpha / transmittance / tile decision has to fall the same way in fp32
    for case in R.DEPTH_CASES:
        scene, cam = R.depth_case(case)
        m = D.scene_margins(*scene, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, case[2], case[3])
        assert min(v for k, v in m.items() if k != "depth_gap") >= D.SCENE_MARGIN, (case, m)
        assert m["depth_gap"] >= D.DEPTH_GAP_MARGIN, (case, m)
        if case[0] == "deep":
            assert m["transmittance"] >= D.DEEP_T_MARGIN, (case, m)


def test_deep_depth_case_covers_batches_saturation_and_early_stop():
    case = [c for c in R.DEPTH_CASES if c[0] == "deep"][0]
    scene, cam = R.depth_case(case)
    _, pr = D.render(*scene, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, case[2], case[3], [0, 0, 0])
    assert int(pr["list_len"].max()) > 2 * 256                                  # tile lists of more than two LDS batches
    assert int(pr["saturated"].sum()) > 0                                       # pixels that stop on the transmittance floor
    assert bool((pr["n_contrib"] + 256 < pr["list_len"]).any())                 # ... a whole batch before their list ends
    da = R.depth_alpha(scene, cam, case[2], case[3])
    assert torch.equal(da["n_contrib"], pr["n_contrib"])                        # the vectorised restatement stops where the dense oracle does
    assert float((da["final_T"] - pr["final_T"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", list(R.TSDF_CASES))
def test_tsdf_scene_keeps_its_margins(name):
    """Nearest-pixel rounding, z against 0.2, |sdf| against trunc, alpha against alpha_min and the sign of the mean TSDF are not decided
    within fp32 error outside the excluded voxels, and those are at most 1 % of the volume: the float32 run of the restatement then makes
    every decision as the fp64 run does.  Every case but the default also leaves the kernel by each of its ways (the default never by z <= 0.2)."""
    case = R.sphere_tsdf_case(**R.TSDF_CASES[name])
    vol, near = R.sphere_tsdf_restatement(case)
    share = float(near.double().mean())
    print(f"excluded share {share:.4%}")
    assert share <= R.MAX_EXCLUDED, share
    counts = R.tsdf_branch_counts(*R.sphere_tsdf_views(case))
    print(counts)
    if name == "default":
        assert float((vol["weight"] > 0).double().mean()) > 0.9 and vol["weight"].max() == len(case["cams"])
        assert counts["near_plane"] == 0 and min(v for k, v in counts.items() if k != "near_plane") > 0
    else:
        assert case["N"] ** 3 % 256 != 0 and case["cams"][0].width != case["cams"][0].height
        assert min(counts.values()) > 0, counts
        assert vol["trunc"] == 0.4 != 4 * 2 * case["bound"] / case["N"]
    inside = (vol["weight"] > 0) & (vol["tsdf_sum"] < 0)
    assert 50 < int(inside.sum()) < case["N"] ** 3 // 8                         # a surface: some voxels inside, most outside
    vol32, _ = R.sphere_tsdf_restatement(case, torch.float32)
    keep = ~near
    assert torch.equal(vol32["weight"].double()[keep], vol["weight"][keep])
    assert torch.equal(vol32["rgb_weight"].double()[keep], vol["rgb_weight"][keep])
    mean64, mean32 = vol["tsdf_sum"] / vol["weight"].clamp_min(1), vol32["tsdf_sum"].double() / vol32["weight"].double().clamp_min(1)
    err = float((mean32 - mean64)[keep].abs().max())
    print(f"float32 restatement vs fp64, mean TSDF: {err:.3e}")
    assert err <= 1e-5 / 4          # the GPU bar is 1e-5: the number format alone stays well inside it
    assert bool(((mean32 < 0) == (mean64 < 0))[keep].all())


def test_tsdf_canary_case_would_write_the_first_voxel_past_the_volume():
    # tests/test_recon_geom_gpu.py surrounds this case's accumulators with guard elements: a bound check that let linear index N^3 through
    # would have to write there for the guards to notice, and some view does (another case's views all miss that voxel)
    case = R.sphere_tsdf_case(**R.TSDF_CASES[R.TSDF_CANARY_CASE])
    assert case["N"] ** 3 % 256 not in (0, 255) and R.tsdf_phantom_voxel(case) > 0
    assert R.tsdf_phantom_voxel(R.sphere_tsdf_case(**R.TSDF_CASES["n26-40x24"])) == 0


# ---- the volumes of the surface-nets tests ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes():
    """name -> (volume, restatement's extraction of its float32 values promoted to fp64)"""
    vols = {name: make() for name, make in R.MESH_VOLUMES.items()}
    return {name: (vol, R.extract(R.promoted(vol))) for name, vol in vols.items()}


@pytest.mark.parametrize("name", list(R.MESH_VOLUMES))
def test_float32_restatement_extracts_the_same_mesh(meshes, name):
    # every decision of the extraction is the sign of a numerator or a weight against 0: exact in any format.  What is left is the arithmetic
    # of the vertex positions and colours, a few ulp of 1 (the GPU bar is 1e-6)
    vol, (rv, rf, rc, _, _) = meshes[name]
    v32, f32, c32, _, _ = R.extract(vol)
    assert v32.dtype == torch.float32 and rv.dtype == torch.float64 and rv.shape[0] > 0
    assert torch.equal(f32, rf) and v32.shape == rv.shape
    assert float((v32.double() - rv).abs().max()) <= 2.5e-7 and float((c32.double() - rc).abs().max()) <= 2.5e-7


@pytest.mark.parametrize("name, vertices, faces, configurations", [("random13", 1298, 2282, 253), ("random11", 808, 1558, 246)])
def test_random_volumes_cover_the_sign_configurations(meshes, name, vertices, faces, configurations):
    vol, (rv, rf, rc, flags, _) = meshes[name]
    N = vol["N"]
    assert N ** 3 % 256 and (N - 1) ** 3 % 256 and 3 * N ** 3 % 256           # every launch ends in a partial block
    stats = R.cell_stats(vol)
    grey = int((rc == 0.5).all(1).sum())
    print(stats, f"{grey} grey vertices of {rv.shape[0]}, {rf.shape[0]} faces")
    assert stats["configurations"] == configurations >= 246                   # of the 254 mixed ones
    assert stats["refused_unseen"] > 100
    assert grey > 100
    assert bool(((rc >= 0) & (rc <= 1)).all()) and int((rc != 0.5).any(1).sum()) > 100
    assert (rv.shape[0], rf.shape[0]) == (vertices, faces) and int(flags.sum()) == vertices
    assert 0 <= int(rf.min()) and int(rf.max()) < vertices


def test_tiny_random_volumes(meshes):
    for name in ("random6", "random3"):
        vol, (rv, rf, _, flags, _) = meshes[name]
        N = vol["N"]
        M = N - 1
        assert rv.shape[0] > 0 and rf.shape[0] > 0
        cells = torch.nonzero(flags).reshape(-1)
        idx = torch.stack([cells % M, (cells // M) % M, cells // (M * M)], 1)
        if N == 3:
            assert bool(((idx == 0) | (idx == M - 1)).any(1).all())            # every flagged cell touches the border
    vol, (rv, rf, _, flags, _) = meshes["random2"]
    assert rv.shape == (1, 3) and rf.shape == (0, 3) and int(flags.sum()) == 1     # one cell: a vertex and no interior edge


def test_oblique_plane_runs_into_every_face_of_the_volume(meshes):
    vol, (rv, rf, _, _, _) = meshes["plane-oblique"]
    N, bound = vol["N"], vol["bound"]
    voxel = 2 * bound / N
    for d in range(3):          # vertices in the first and in the last layer of cells along every axis
        assert float(rv[:, d].min()) < -bound + 1.5 * voxel and float(rv[:, d].max()) > bound - 1.5 * voxel
    # sign-changing grid edges on the border, which edge_cells has to refuse: the restatement's faces hold none of them
    neg = (vol["tsdf_sum"] < 0).reshape(N, N, N)
    border = 0
    for axis in range(3):       # (tensor dimension 2 - axis)
        a, b = neg.narrow(2 - axis, 0, N - 1), neg.narrow(2 - axis, 1, N - 1)
        cross = a != b
        for other in range(3):
            if other != axis:
                border += int(cross.select(2 - other, 0).sum()) + int(cross.select(2 - other, N - 1).sum())
    assert border > 50, border
    _, cnt, dirsum = R.undirected_counts(rf.numpy())
    assert (cnt <= 2).all() and int((cnt == 1).sum()) > 0 and (dirsum[cnt == 2] == 0).all()
    assert (rv.shape[0], rf.shape[0]) == (285, 502)
    n = torch.tensor([0.3, 0.5, 0.81], dtype=torch.float64)
    assert float((rv @ (n / n.norm()) - 0.05).abs().max()) <= 1e-6              # linear interpolation of a linear field: on the plane


def test_axis_plane_between_two_layers_of_voxels(meshes):
    vol, (rv, rf, _, _, _) = meshes["plane-x"]
    M = vol["N"] - 1
    assert rv.shape[0] == M * M == 121 and rf.shape[0] == 2 * (M - 1) ** 2 == 200
    assert float(rv[:, 0].abs().max()) <= 1e-6
    _, cnt, dirsum = R.undirected_counts(rf.numpy())
    assert (cnt <= 2).all() and (dirsum[cnt == 2] == 0).all() and int((cnt == 1).sum()) == 4 * (M - 1)
    v = rv[rf]
    normal = torch.linalg.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert bool((normal[:, 0] > 0).all())                                       # from the negative side (x < 0) to the positive one


@pytest.mark.parametrize("name, up", [("plane-z-zero", 1.0), ("plane-z-zero-down", -1.0)])
def test_a_mean_of_exactly_zero_counts_as_outside(meshes, name, up):
    """13 voxels a side: the middle layer has z = 0 and a mean TSDF of exactly 0, which is not < 0.  The surface then lies between that layer
    and the negative one beside it, and every crossing interpolates to the zero layer itself: s = m0 / (m0 - 0) = 1 from below (normal
    +z), s = 0 / (0 - m1) = 0 from above (normal -z).  The vertices are at z = 0 (the restatement gives 1.2e-16 and 0)."""
    vol, (rv, rf, _, _, mean) = meshes[name]
    N = vol["N"]
    M = N - 1
    assert int((mean == 0).sum()) == N * N == 169 and bool((mean.reshape(N, N, N)[N // 2] == 0).all())
    assert rv.shape[0] == M * M == 144 and rf.shape[0] == 2 * (M - 1) ** 2 == 242
    assert float(rv[:, 2].abs().max()) <= 1e-6
    v = rv[rf]
    normal = torch.linalg.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert bool((normal[:, 2] * up > 0).all())
