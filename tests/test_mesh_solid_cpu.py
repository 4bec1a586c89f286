"""The winding number, the signed distance and the mesh-to-volume stage of libv3d_recon.so (csrc_recon/meshsolid.hip,
v3d_amd/recon/mesh_solid.py, scripts/pub/solidify_mesh.py) without a GPU: header, ctypes table and exports agree, bad arguments are refused
before any launch, the torch restatement (tests/mesh_solid_ref.py) is honest on cases with known answers, the script's options, the host
API's refusals, and the premises of the cases of tests/test_mesh_solid_gpu.py on the restatement alone."""
import importlib.util
import math
import os
import re

import pytest
import torch

import mesh_bake_ref as B
import mesh_render_ref as M
import mesh_solid_ref as S
import recon_geom_ref as R
from v3d_amd.recon import mesh_solid as MS                                      # (without the feature: the import fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLID_ENTRIES = {"v3d_recon_bvh_moment_round", "v3d_recon_bvh_winding", "v3d_recon_sdf_grid"}
F64, F32 = torch.float64, torch.float32
INF, NAN = float("inf"), float("nan")


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
    assert SOLID_ENTRIES <= declared and declared == set(geometry.SIGNATURES)
    for name in SOLID_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert int(re.search(r"#define V3D_RECON_ABI_VERSION (\d+)", hdr).group(1)) == 1
    for text in ("Mesh solid", "THE WINDING NUMBER", "THE MOMENTS", "THE SUM"):
        assert text in hdr, text
    assert hdr.index("---- Mesh queries") < hdr.index("---- Mesh solid")
    csrc = os.path.join(ROOT, "v3d_amd", "csrc_recon")
    src = open(os.path.join(csrc, "meshsolid.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")
    assert '#include "bvh_walk.h"' in src
    assert src.count("__launch_bounds__(BT)") == 3 and "__launch_bounds__(NT)" not in src          # one wave to a block, every kernel
    assert src.count("__shared__ int stack[STACK * BT]") == 2
    # the closest-point walk is shared, not copied: one definition, in the header the sources include
    walk, query = open(os.path.join(csrc, "bvh_walk.h")).read(), open(os.path.join(csrc, "meshquery.hip")).read()
    for name in ("struct Near", "float box_d2(", "bool beyond(", "bool no_area(", "void near_triangle(", "Near closest_point(", "float dot3(", "NEAR_SLACK ="):
        assert walk.count(name) == 1 and name not in query and name not in src, name


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731

    def calls(fn, names, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in names])

    big = 2 ** 30 + 1
    tree = ("left", "right", "order", "lo", "hi", "verts", "V", "faces", "F")
    tree_defaults = dict(left=p, right=p, order=p, lo=p, hi=p, verts=p, V=162, faces=p, F=320)

    def tree_refusals(call, name):
        for k in ("left", "right", "order", "lo", "hi", "verts", "faces"):
            assert call(**{k: None}) == -1 and name in err() and "null" in err(), k
        assert call(V=0) == -1 and "num_verts" in err()
        assert call(F=0) == -1 and "num_faces 0" in err()
        assert call(F=big) == -1 and "num_faces" in err()

    mr = calls(lib.v3d_recon_bvh_moment_round, tree + ("done_in", "done_out", "mom", "changed", "stream"),
               done_in=p, done_out=p + 0x10000, mom=p, changed=p, stream=None, **tree_defaults)
    for k in ("done_in", "done_out", "mom", "changed"):
        assert mr(**{k: None}) == -1 and "v3d_recon_bvh_moment_round" in err() and "null" in err(), k
    tree_refusals(mr, "v3d_recon_bvh_moment_round")
    assert mr(done_out=p) == -1 and "two buffers" in err()
    wn = calls(lib.v3d_recon_bvh_winding, ("points", "N", "beta") + tree + ("mom", "w", "stream"),
               points=p, N=100, beta=2.0, mom=p, w=p, stream=None, **tree_defaults)
    for k in ("points", "mom", "w"):
        assert wn(**{k: None}) == -1 and "v3d_recon_bvh_winding" in err() and "null" in err(), k
    tree_refusals(wn, "v3d_recon_bvh_winding")
    assert wn(N=0) == -1 and "num_points" in err()
    assert wn(N=-1) == -1 and "num_points" in err()
    for bad in (-1.0, NAN, INF):
        assert wn(beta=bad) == -1 and "beta" in err(), bad
    sg = calls(lib.v3d_recon_sdf_grid, tree + ("mom", "colors", "N", "bound", "trunc", "beta", "ts", "w", "rs", "rw", "stream"),
               mom=p, colors=None, N=24, bound=0.7, trunc=0.2, beta=2.0, ts=p, w=p, rs=p, rw=p, stream=None, **tree_defaults)
    for k in ("mom", "ts", "w", "rs", "rw"):
        assert sg(**{k: None}) == -1 and "v3d_recon_sdf_grid" in err() and "null" in err(), k
    tree_refusals(sg, "v3d_recon_sdf_grid")
    for bad in (1, 0, -4, 513):
        assert sg(N=bad) == -1 and f"resolution {bad}" in err(), bad
    for bad in (0.0, -1.0, NAN, INF):
        assert sg(bound=bad) == -1 and "bound" in err(), bad
        assert sg(trunc=bad) == -1 and "trunc" in err(), bad
    for bad in (-1.0, NAN, INF):
        assert sg(beta=bad) == -1 and "beta" in err(), bad


# ---- the restatement is honest ----------------------------------------------------------------------------------------------------------------
def test_winding_of_closed_reversed_and_nested_spheres():
    g = torch.Generator().manual_seed(0)
    sph = torch.nn.functional.normalize(torch.randn(60, 3, generator=g, dtype=F64), dim=1)
    inner, inside, outside = sph[:20] * 0.15, sph[20:40] * 0.3, sph[40:] * 0.9                  # in both spheres, between them, outside
    for kind, expect in (("closed", (1, 1, 0)), ("reversed", (-1, -1, 0)), ("nested", (2, 1, 0)), ("nested-reversed", (0, 1, 0))):
        v, f = S.mesh(kind)
        for pts, e in zip((inner, inside, outside), expect):
            w = S.exact_winding(v, f, pts)
            assert float((w - e).abs().max()) < 1e-12, (kind, e)
    v, f = S.mesh("closed")
    assert float((S.exact_winding(v, f, inside, F32).double() - 1).abs().max()) < 1e-5
    nan = S.exact_winding(v, f, torch.tensor([[0.0, NAN, 0.0], [INF, 0.0, 0.0]]))
    assert bool(torch.isnan(nan).all())


def hemisphere(segments=16, rings=4):
    """A latitude-longitude hemisphere of the unit sphere over z >= 0, wound outward; its rim lies exactly in the plane z = 0"""
    v = [[0.0, 0.0, 1.0]]
    for r in range(1, rings + 1):
        th = 0.5 * math.pi * r / rings
        z = 0.0 if r == rings else math.cos(th)
        v += [[math.sin(th) * math.cos(2 * math.pi * k / segments), math.sin(th) * math.sin(2 * math.pi * k / segments), z] for k in range(segments)]
    ring = lambda r, k: 1 + (r - 1) * segments + k % segments  # noqa: E731
    f = [[0, ring(1, k), ring(1, k + 1)] for k in range(segments)]
    for r in range(1, rings):
        for k in range(segments):
            f += [[ring(r, k), ring(r + 1, k), ring(r + 1, k + 1)], [ring(r, k), ring(r + 1, k + 1), ring(r, k + 1)]]
    return torch.tensor(v, dtype=F64), torch.tensor(f), [ring(rings, k) for k in range(segments)]


def test_half_at_the_centre_of_a_hemispheres_rim_and_the_in_plane_rule():
    # By hand: the rim lies in a plane through the query, so the hemisphere fills exactly one side of it: 2 pi of 4 pi, whatever the
    # triangulation.  The flat disc on the rim closes the solid; seen from its own centre every one of its triangles lies in the query's
    # plane, num == 0, and adds nothing: the cap of a flat hole sits where w = 0.5.
    v, f, rim = hemisphere()
    assert float(S.exact_winding(v, f, torch.zeros(1, 3, dtype=F64), F64)[0]) == pytest.approx(0.5, abs=1e-14)
    assert float(S.exact_winding(v, f, torch.tensor([[0.0, 0.0, 0.2]], dtype=F64))[0]) > 0.5
    assert float(S.exact_winding(v, f, torch.tensor([[0.0, 0.0, -0.2]], dtype=F64))[0]) < 0.5
    centre = v.shape[0]
    vd = torch.cat([v, torch.zeros(1, 3, dtype=F64)])
    disc = torch.tensor([[centre, rim[(k + 1) % len(rim)], rim[k]] for k in range(len(rim))])
    closed = torch.cat([f, disc])
    assert float(S.exact_winding(vd, closed, torch.tensor([[0.3, 0.1, 0.0]], dtype=F64))[0]) == pytest.approx(0.5, abs=1e-14)      # on the disc: its Omega is 0
    assert float(S.exact_winding(vd, closed, torch.tensor([[0.1, 0.1, 0.3]], dtype=F64))[0]) == pytest.approx(1.0, abs=1e-12)
    assert float(S.exact_winding(vd, closed, torch.tensor([[0.1, 0.1, -0.3]], dtype=F64))[0]) == pytest.approx(0.0, abs=1e-12)
    # the rule itself: without it a query ON the triangle would get atan2(0, den < 0) = pi, Omega = 2 pi
    tv, tf = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2]])
    q = torch.tensor([[0.25, 0.25, 0.0], [2.0, 2.0, 0.0], [-1.0, 0.5, 0.0]])
    for dt in (F64, F32):
        assert S.solid_angles(tv, tf, q, dt).reshape(-1).tolist() == [0.0, 0.0, 0.0]
    above = S.solid_angles(tv, tf, torch.tensor([[0.25, 0.25, 1e-3]]))
    assert abs(abs(float(above)) - 2 * math.pi) < 0.05                       # just off the plane: nearly the half space, and signed


def test_exactly_half_counts_as_inside():
    v, f = S.half_octahedron()
    o = torch.zeros(1, 3)
    assert float(S.exact_winding(v, f, o)[0]) == pytest.approx(0.5, abs=1e-15)
    assert S.exact_winding(v, f, o, F32).tolist() == [0.5]                       # float: exactly
    tree = S.build_tree(v, f)
    N, bound = S.HALF_GRID["N"], S.HALF_GRID["bound"]
    assert S.voxel_centres32(N, bound)[13].tolist() == [0.0, 0.0, 0.0]
    vol = S.sdf_volume(tree, S.moments(tree, v, f, F32), v, f, None, N, bound, 1.0, 0.0, F32)
    assert float(vol["w"][13]) == 0.5 and float(vol["tsdf_sum"][13]) < 0         # w >= 0.5 is inside; `>` would leave it outside


def test_moments_of_the_root_and_the_radius_bound():
    for kind in ("closed", "open", "nested"):
        v, f, tree, m64, m32 = S.cpu_case(kind)
        F = f.shape[0]
        assert abs(float(m64[0, 7]) - S.mesh_area(v, f)) < 1e-12
        if kind != "open":
            assert float(m64[0, :3].abs().max()) < 1e-12                        # a closed mesh's area vectors sum to 0
        else:
            assert float(m64[0, 2]) < -0.1                                      # the missing cap looked up
        assert float((m32.double() - m64).abs().max()) < 1e-6
        order, vd = tree["order"], v.double()
        leaves = {}
        for n, _ in reversed(S.preorder(tree, F)):
            leaves[n] = [int(order[n - (F - 1)])] if n >= F - 1 else leaves[int(tree["left"][n])] + leaves[int(tree["right"][n])]
        for n in range(0, 2 * F - 1, 7):
            pts = vd[f[torch.tensor(leaves[n])].reshape(-1)]
            assert float(((pts - m64[n, 4:7]) ** 2).sum(1).max()) <= float(m64[n, 3]) * (1 + 1e-12) + 1e-15, n
    # the faces that are none: a zero-area face has area 0 and a centroid, a face with index V is all zeros
    v, f = B.degenerate_mesh()
    tree = S.build_tree(v, f)
    m = S.moments(tree, v, f)
    F = f.shape[0]
    leaf = {int(face): F - 1 + k for k, face in enumerate(tree["order"].tolist())}
    assert float(m[leaf[320], 7]) == 0 and float(m[leaf[320], :3].abs().max()) == 0 and float(m[leaf[320], 4:7].abs().max()) > 0
    assert not m[leaf[321]].any()
    assert abs(float(m[0, 7]) - S.mesh_area(v[:], f[:320])) < 1e-12
    # one face
    v1, f1 = v, f[:1]
    t1 = S.build_tree(v1, f1)
    assert t1["left"].tolist() == [-1] and tuple(S.moments(t1, v1, f1).shape) == (1, 8)


@pytest.mark.parametrize("kind", ("closed", "open", "nested"))
def test_tree_sum_is_exact_at_beta_0_and_close_at_2_and_3(kind):
    v, f, tree, m64, m32 = S.cpu_case(kind)
    q = S.queries()
    exact = S.exact_winding(v, f, q)
    w0, gap0, visited = S.tree_sum(tree, m64, v, f, q, 0.0)
    assert float((w0 - exact).abs().max()) < 1e-13 and bool(torch.isinf(gap0).all()) and int(visited.min()) == 2 * f.shape[0] - 1
    dev = {}
    for beta in S.BETAS:
        w, gap, w32 = S.cpu_winding(kind, beta)
        keep = gap >= S.GAP
        dev[beta] = float((w - exact)[keep].abs().max())
        print(f"{kind} beta {beta:g}: |w - exact| max {dev[beta]:.3e} mean {float((w - exact)[keep].abs().mean()):.3e}; float32 against fp64 "
              f"{float((w32.double() - w)[keep].abs().max()):.3e}; {int((~keep).sum())} of {q.shape[0]} left out")
        assert not bool(((w >= 0.5) != (exact >= 0.5))[keep].any())              # no query changes side
        assert dev[beta] < float((exact - 0.5).abs().min())                      # ... and none could have: the queries keep clear of 0.5
    assert dev[3.0] < dev[2.0]


# ---- the premises of the GPU cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("closed", "open", "nested"))
def test_premises_of_the_winding_cases(kind):
    v, f = S.mesh(kind)
    q = S.queries()
    assert q.shape[0] == 1100 and S.COUNTS == (1, 63, 64, 65, 1100)
    assert float(S.surface_distance(kind).min()) >= S.SURFACE_MARGIN * S.diagonal(v)
    lo, hi = v.min(0).values, v.max(0).values
    for k in range(3):                                                           # beyond the root box on every side
        assert bool((q[:, k] < lo[k] - 0.3).any()) and bool((q[:, k] > hi[k] + 0.3).any())
    w = S.exact_winding(v, f, q)
    for n in S.COUNTS:                                                           # every prefix holds both sides (but the first query alone)
        assert n == 1 or (bool((w[:n] > 0.75).any()) and bool((w[:n] < 0.25).any()))
    for beta in S.BETAS:
        _, gap, _ = S.cpu_winding(kind, beta)
        for n in S.COUNTS:
            assert S.excluded_share(gap[:n] >= S.GAP) <= S.EXCLUDE_MAX, (beta, n)


@pytest.mark.parametrize("case", S.GRID_CASES[:4], ids=S.grid_case_id)
def test_premises_of_the_volume_cases(case):
    kind, N, bound, _ = case
    v, f = S.mesh(kind)
    r64, r32 = S.cpu_volume(case)
    trunc = S.grid_trunc(N, bound)
    assert float(r64["dist"].min()) >= S.SURFACE_MARGIN * S.diagonal(v)
    mask = S.volume_mask(r64, r32, trunc)
    assert S.excluded_share(mask) <= S.EXCLUDE_MAX
    assert not bool(((r32["tsdf_sum"] < 0) != (r64["tsdf_sum"] < 0))[mask].any())
    assert bool((r64["tsdf_sum"] < 0).any()) and bool((r64["tsdf_sum"] > 0).any())
    if N > 8:                                                                    # (at N = 8 the band of 4 voxels fills the volume: every voxel hits)
        assert bool((r64["tsdf_sum"] == 1).any()) and bool(torch.isinf(r64["dist"]).any())
    if N % 4:
        assert (N + 3) // 4 * 4 > N                                              # partial bricks on every axis
    assert bool((r64["rgb_weight"] == torch.isfinite(r64["dist"]).double()).all())


def e2e_cpu(kind, dtype=F64):
    v, f, tree, m64, m32 = S.cpu_case(kind)
    N, bound = S.E2E["N"], S.E2E["bound"]
    vol = S.sdf_volume(tree, m64 if dtype == F64 else m32, v, f, M.position_colors(v), N, bound, S.grid_trunc(N, bound), S.GRID_BETA, dtype)
    return R.extract(vol)


@pytest.mark.parametrize("kind", ("closed", "open"))
def test_end_to_end_on_the_restatement_closes_the_sphere(kind):
    v, f = S.mesh(kind)
    und, cnt, _ = R.undirected_counts(f.numpy())
    assert (kind == "open") == bool((cnt == 1).any())
    ov, of, oc, _, _ = e2e_cpu(kind)
    und, cnt, ssum = R.undirected_counts(of.numpy())
    assert bool((cnt == 2).all()) and not ssum.any()                             # every directed edge once and its reverse once
    assert ov.shape[0] - und.shape[0] + of.shape[0] == 2
    assert R.signed_volume(ov.numpy(), of.numpy()) > 0
    ov32 = e2e_cpu(kind, F32)[0]
    print(f"{kind}: {ov.shape[0]} vertices, {of.shape[0]} faces; Chamfer float32 against fp64 {R.chamfer(ov32, ov):.3e}")
    if kind == "open":
        voxel = 2.0 * S.E2E["bound"] / S.E2E["N"]
        cap = S.cap_vertices(ov, v, f, voxel)
        zlo, zhi = S.rim_heights()
        z = ov[cap][:, 2]
        assert int(cap.sum()) > 10
        # the GPU test grants two voxels of margin; the restatement stays within half of that
        assert float(z.min()) >= zlo - voxel and float(z.max()) <= zhi + voxel, (float(z.min()), float(z.max()), zlo, zhi)


def test_the_reversed_sphere_has_no_inside():
    v, f, tree, m64, _ = S.cpu_case("reversed")
    N, bound = 12, 0.7
    vol = S.sdf_volume(tree, m64, v, f, None, N, bound, S.grid_trunc(N, bound), S.GRID_BETA)
    assert not bool((vol["tsdf_sum"] < 0).any()) and not vol["rgb_weight"].any() and not vol["rgb_sum"].any()
    assert R.extract(vol)[1].shape[0] == 0


# ---- the script and the host API --------------------------------------------------------------------------------------------------------------
def _script():
    spec = importlib.util.spec_from_file_location("solidify_mesh_script", os.path.join(ROOT, "scripts", "pub", "solidify_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_and_refusals(capsys):
    mod = _script()
    a = mod.build_parser().parse_args(["--mesh", "x.ply", "-o", "y.ply"])
    assert (a.resolution, a.beta, a.smooth, a.flip, a.json, a.render_orbit, a.white_background, a.bound, a.trunc) == (256, 2.0, 0, False, None, 0, False,
                                                                                                                      None, None)
    a = mod.build_parser().parse_args(["--mesh", "x.ply", "-o", "y.ply", "--resolution", "64", "--beta", "3", "--smooth", "5", "--flip", "--json", "s.json",
                                       "--render_orbit", "4", "-w"])
    assert (a.resolution, a.beta, a.smooth, a.flip, a.json, a.render_orbit, a.white_background) == (64, 3.0, 5, True, "s.json", 4, True)
    base = ["--mesh", "/nonexistent/x.ply", "-o", "/nonexistent/y.ply"]
    for bad in (["--resolution", "1"], ["--resolution", "513"], ["--beta", "-1"], ["--beta", "nan"], ["--beta", "inf"], ["--smooth", "-1"],
                ["--render_orbit", "-1"], ["--bound", "0"], ["--trunc", "-1"], ["--trunc", "inf"], ["--reso", "0"], ["--reso", "5000"]):
        with pytest.raises(SystemExit):                                          # before the mesh is read or a GPU touched
            mod.main(base + bad)
    with pytest.raises(SystemExit):
        mod.main(["-o", "y.ply"])
    capsys.readouterr()
    assert mod.MAX_RESOLUTION == MS.MAX_RESOLUTION == 512


def test_host_api_refusals_before_any_launch():
    v, f = S.mesh("small")
    c = M.position_colors(v)
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError, match="beta"):
            MS.mesh_to_volume(v, f, beta=bad, device="cpu")
        with pytest.raises(ValueError, match="beta"):
            MS.solidify_mesh(v, f, c, beta=bad, device="cpu")
    for bad in (1, 513):
        with pytest.raises(ValueError, match="resolution"):
            MS.mesh_to_volume(v, f, resolution=bad, device="cpu")
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="bound"):
            MS.mesh_to_volume(v, f, bound=bad, device="cpu")
        with pytest.raises(ValueError, match="trunc"):
            MS.solidify_mesh(v, f, c, trunc=bad, device="cpu")
    with pytest.raises(ValueError, match="nothing to hit"):
        MS.mesh_to_volume(v, f[:0], device="cpu")
    with pytest.raises(ValueError, match="bounds nothing"):
        MS.solidify_mesh(v, f[:0], c, device="cpu")
    with pytest.raises(ValueError, match="colours"):
        MS.mesh_to_volume(v, f, c[:-1], resolution=8, device="cpu")
    with pytest.raises(ValueError, match="smooth"):
        MS.solidify_mesh(v, f, c, smooth=-1, device="cpu")
    with pytest.raises(ValueError, match="face index"):
        MS.solidify_mesh(v, f + 1, c, device="cpu")
    assert "ORIENTATION MATTERS" in MS.__doc__ and "flip" in MS.solidify_mesh.__doc__ and "wound inward" in MS.solidify_mesh.__doc__
    # the defaults of the volume
    b, t = MS.default_volume(v, 256)
    m = 1.1 * float(v.abs().max())
    assert t == pytest.approx(8.0 * b / 256) and b == pytest.approx(m + 8.0 * m / 256)
    assert MS.default_volume(v, 64, trunc=0.05) == (pytest.approx(m + 0.05), 0.05)
    assert MS.default_volume(v, 64, bound=1.0) == (1.0, pytest.approx(0.125))
    # the voxel centres are the kernel's floats: the exact value rounded once
    assert torch.equal(MS.voxel_centres(22, 0.71, "cpu"), S.voxel_centres32(22, 0.71))
    assert float((MS.voxel_centres(22, 0.71, "cpu").double() - R.voxel_centres(22, 0.71)).abs().max()) < 1e-6
    # the torch measures
    assert MS.edge_counts(f, v.shape[0]) == (480, 0) and MS.edge_counts(S.mesh("open")[1], 642)[1] > 0
    assert MS.signed_volume(v, f) == pytest.approx(R.signed_volume(v.numpy(), f.numpy()), rel=1e-12)
