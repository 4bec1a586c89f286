"""The gfx950 winding number, signed distance and mesh-to-volume stage (csrc_recon/meshsolid.hip, v3d_amd/recon/mesh_solid.py,
scripts/pub/solidify_mesh.py) against the torch restatement (tests/mesh_solid_ref.py): every row of the moments, the winding number against
the brute force (beta = 0) and against the walk restated on the DEVICE's own tree and moments (beta = 2, 3: each kernel on its own inputs),
the volume, the signed distance, guards around every output, and a sphere, closed and open, through the whole stage.

The bar for continuous outputs is the project's standing one: the kernel may be off from the fp64 restatement by 4x what the restatement's
own float32 run is off, the float32 figure taken over the whole case, once.  A query is left out of a tree-mode comparison only when a far
decision it took was closer than 1e-5 (relative), a voxel also where the fp64 w is within the bar of 0.5 or its distance within the bar of
trunc; at most 2 % of a case, asserted here on the device's tree as tests/test_mesh_solid_cpu.py asserts it on the restatement's."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_bake_ref as B
import mesh_render_ref as M
import mesh_solid_ref as S
import recon_geom_ref as R
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_bake as MB
from v3d_amd.recon import mesh_query as MQ
from v3d_amd.recon import mesh_solid as MS

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
INF, NAN = float("inf"), float("nan")
GUARD = 4096


class Guarded:
    """An output of n elements with GUARD sentinel elements before and after it"""

    def __init__(self, n, sentinel=-7.0):
        self.n, self.sentinel = n, sentinel
        self.buf = torch.full((2 * GUARD + n,), sentinel, dtype=F32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * 4

    def take(self):
        assert bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.n:] == self.sentinel).all()), "a guard was written"
        return self.buf[GUARD:GUARD + self.n].clone()


@functools.lru_cache(maxsize=None)
def device_case(kind):
    """(verts, faces, bvh, moments, rounds, host tree, host moments, fp64 and float32 restated moments ON THE DEVICE'S TREE): once per mesh"""
    v, f = S.mesh(kind)
    bvh = MB.build_bvh(v, f)
    mom, rounds = MS._moments(bvh)
    tree = S.host_tree(bvh)
    return v, f, bvh, mom, rounds, tree, mom.cpu(), S.moments(tree, v, f), S.moments(tree, v, f, F32)


# ---- 1. the moments ---------------------------------------------------------------------------------------------------------------------------
def moment_meshes():
    v, f = S.mesh("small")
    yield "sphere320", v, f
    yield "one", v, f[:1]
    yield "two", v, f[:2]
    yield "f257", v, f[:257]
    yield "degenerate", *B.degenerate_mesh()
    yield "strip", *B.low_bit_strip()


@pytest.mark.parametrize("name", [m[0] for m in moment_meshes()])
def test_moments_match_the_restatement_on_every_row(name):
    v, f = next((a, b) for n, a, b in moment_meshes() if n == name)
    F = f.shape[0]
    bvh = MB.build_bvh(v, f)
    mom, rounds = MS._moments(bvh)
    assert tuple(mom.shape) == (2 * F - 1, 8) and mom.dtype == F32
    assert 1 <= rounds <= MB.height_bound(F) + 8 and (F > 1 or rounds == 1)
    tree = S.host_tree(bvh)
    r64, r32 = S.moments(tree, v, f), S.moments(tree, v, f, F32)
    scale = torch.tensor([S.mesh_area(v, f[:320] if name == "degenerate" else f)] * 3 + [S.diagonal(v) ** 2] + [S.diagonal(v)] * 3 +
                         [S.mesh_area(v, f[:320] if name == "degenerate" else f)], dtype=F64)
    err = float(((mom.cpu().double() - r64).abs() / scale).max())
    bar = 4 * float(((r32.double() - r64).abs() / scale).max())
    print(f"{name}: F {F}, {rounds} rounds: moments off by {err:.3e} of the mesh's area / diagonal (bar {bar:.3e})")
    record_parity(f"mesh_solid_moments[{name}]", {"max_rel": err, "bar": bar, "rounds": rounds})
    assert err <= bar
    assert torch.equal(mom.cpu()[:, 7] == 0, r64[:, 7] == 0)                     # the rows the walk skips
    # `done` everywhere: one more round changes nothing, and two runs are bit-equal
    assert torch.equal(MS.node_moments(bvh), mom)
    if name == "degenerate":
        leaf = {int(face): F - 1 + k for k, face in enumerate(tree["order"].tolist())}
        assert not mom[leaf[321]].any() and float(mom[leaf[320], 7]) == 0


# ---- 2. the winding number --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("closed", "open", "nested"))
def test_winding_matches_the_brute_force_and_the_restated_walk(kind):
    v, f, bvh, mom, _, tree, mom_host, m64, m32 = device_case(kind)
    q = S.queries()
    ref = {0.0: (S.exact_winding(v, f, q), torch.full((q.shape[0],), INF, dtype=F64), S.exact_winding(v, f, q, F32))}
    for beta in S.BETAS:                                  # the walk on the device's tree with the device's moments, in fp64 and in float32
        w, gap, _ = S.tree_sum(tree, mom_host.double(), v, f, q, beta)
        ref[beta] = (w, gap, S.tree_sum(tree, mom_host, v, f, q, beta, F32)[0])
    lib = G.load_library()
    for beta, (w64, gap, w32) in ref.items():
        keep_all = gap >= S.GAP
        bar = 4 * float((w32.double() - w64)[keep_all].abs().max())
        for n in S.COUNTS:
            got = MS.winding_numbers(bvh, q[:n], beta, mom)
            assert got.dtype == F32 and tuple(got.shape) == (n,)
            keep = keep_all[:n]
            assert S.excluded_share(keep) <= S.EXCLUDE_MAX, (beta, n)
            err = float((got.cpu().double() - w64[:n])[keep].abs().max())
            assert err <= bar, (kind, beta, n, err, bar)
            assert torch.equal(MS.winding_numbers(bvh, q[:n], beta, mom), got), "two runs differ"
            if n in (65, 1100):
                out, qd = Guarded(n), q[:n].to(DEV).contiguous()
                G._check(lib, lib.v3d_recon_bvh_winding(qd.data_ptr(), n, beta, *bvh._args(), mom.data_ptr(), out.ptr, G._stream()), "winding")
                assert torch.equal(out.take(), got)
        print(f"{kind} beta {beta:g}: w off by {err:.3e} (bar {bar:.3e}); {int((~keep_all).sum())} of 1100 left out")
        record_parity(f"mesh_solid_winding[{kind}-beta{beta:g}]", {"max_abs": err, "bar": bar, "left_out": int((~keep_all).sum())})
    # the tree sum against the exact one, on the device: for the record, and no query changes side
    exact = ref[0.0][0]
    for beta in S.BETAS:
        got = MS.winding_numbers(bvh, q, beta, mom).cpu().double()
        assert torch.equal(got >= 0.5, exact >= 0.5)
        record_parity(f"mesh_solid_tree_against_exact[{kind}-beta{beta:g}]", {"max_abs": float((got - exact).abs().max()), "mean_abs": float((got - exact).abs().mean())})


def test_winding_at_vertices_on_faces_nan_queries_and_one_face():
    v, f, bvh, mom, *_ = device_case("open")
    on_face = v[f[:100]].mean(1)
    nan = torch.tensor([[0.0, NAN, 0.0], [INF, 0.0, 0.0], [0.0, 0.0, -INF]])
    p = torch.cat([v[:100], on_face, nan, torch.zeros(1, 3)])
    for beta in (0.0, 2.0):
        w = MS.winding_numbers(bvh, p, beta, mom)
        assert bool(torch.isfinite(w[:200]).all()) and bool(torch.isnan(w[200:203]).all())
        assert abs(float(w[203]) - float(S.exact_winding(v, f, torch.zeros(1, 3))[0])) < 0.05
        assert torch.equal(w[:200], MS.winding_numbers(bvh, p, beta, mom)[:200]), "two runs differ"
    assert torch.equal(torch.isnan(MS.winding_numbers(bvh, p, 2.0)), torch.isnan(w))                 # moments=None: computed inside
    assert tuple(MS.winding_numbers(bvh, torch.zeros(0, 3), 2.0).shape) == (0,)
    # one face: the lone leaf is the root
    tv = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    one = MB.build_bvh(tv, torch.tensor([[0, 1, 2]]))
    q = torch.tensor([[0.2, 0.2, 0.5], [0.2, 0.2, -0.5], [0.25, 0.25, 0.0], [3.0, 3.0, 0.0], [5.0, 4.0, 3.0]])
    ref = S.exact_winding(tv, torch.tensor([[0, 1, 2]]), q)
    for beta in (0.0, 2.0):
        w = MS.winding_numbers(one, q, beta).cpu().double()
        assert float((w - ref)[:4].abs().max()) < 1e-6 and w[2:4].tolist() == [0.0, 0.0]              # in the plane: exactly 0
        assert abs(float(w[4] - ref[4])) < (1e-6 if beta == 0 else 1e-3)
    with pytest.raises(ValueError, match="moments"):
        MS.winding_numbers(bvh, p, 2.0, mom[:-1])


# ---- 3. the volume and the signed distance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.GRID_CASES, ids=S.grid_case_id)
def test_sdf_grid_matches_the_restatement(case):
    kind, N, bound, rgb = case
    v, f, bvh, mom, _, tree, mom_host, _, _ = device_case(kind)
    trunc, beta = S.grid_trunc(N, bound), S.GRID_BETA
    c = M.position_colors(v) if rgb else None
    r64 = S.sdf_volume(tree, mom_host.double(), v, f, c, N, bound, trunc, beta)
    r32 = S.sdf_volume(tree, mom_host, v, f, c, N, bound, trunc, beta, F32)
    mask = S.volume_mask(r64, r32, trunc)
    assert S.excluded_share(mask) <= S.EXCLUDE_MAX
    cd = c.to(DEV).contiguous() if rgb else None
    n3 = N ** 3
    outs = [Guarded(n3), Guarded(n3), Guarded(3 * n3), Guarded(n3)]
    lib = G.load_library()
    G._check(lib, lib.v3d_recon_sdf_grid(*bvh._args(), mom.data_ptr(), cd.data_ptr() if rgb else None, N, bound, trunc, beta, *[o.ptr for o in outs],
                                         G._stream()), "sdf_grid")
    ts, wt, rs, rw = (o.take().cpu() for o in outs)
    assert bool((wt == 1).all())
    assert torch.equal(ts[mask] < 0, r64["tsdf_sum"][mask] < 0)
    err = float((ts.double() - r64["tsdf_sum"])[mask].abs().max())
    bar = 4 * float((r32["tsdf_sum"].double() - r64["tsdf_sum"])[mask].abs().max())
    hit = torch.isfinite(r64["dist"])
    assert torch.equal(rw[mask], (hit if rgb else torch.zeros_like(hit)).float()[mask])
    rgb_err = float((rs.reshape(3, n3).double() - r64["rgb_sum"])[:, mask].abs().max())
    rgb_bar = 4 * float((r32["rgb_sum"].double() - r64["rgb_sum"])[:, mask].abs().max())
    print(f"{S.grid_case_id(case)}: tsdf off by {err:.3e} (bar {bar:.3e}), colours by {rgb_err:.3e} (bar {rgb_bar:.3e}); "
          f"{int((~mask).sum())} of {n3} voxels left out")
    record_parity(f"mesh_solid_grid[{S.grid_case_id(case)}]", {"tsdf_max_abs": err, "tsdf_bar": bar, "rgb_max_abs": rgb_err, "rgb_bar": rgb_bar,
                                                              "left_out": int((~mask).sum())})
    assert err <= bar and rgb_err <= rgb_bar
    if not rgb:
        assert not rs.any() and not rw.any()
    # the public call: the same bits, twice
    vol = MS._fill(bvh, mom, cd, N, bound, trunc, beta)
    again = MS._fill(bvh, mom, cd, N, bound, trunc, beta)
    for a, b, o in zip((vol.tsdf_sum, vol.weight, vol.rgb_sum, vol.rgb_weight), (again.tsdf_sum, again.weight, again.rgb_sum, again.rgb_weight), (ts, wt, rs, rw)):
        assert torch.equal(a, b) and torch.equal(a.reshape(-1).cpu(), o)
    # ... and signed_distances on the voxel centres, bit for bit: the same device functions
    p = MS.voxel_centres(N, bound, DEV)
    assert torch.equal(p.cpu(), S.voxel_centres32(N, bound))
    sd = MS.signed_distances(bvh, p, beta, trunc, mom)
    found = sd["face"] >= 0
    s = torch.where(sd["w"] >= 0.5, -1.0, 1.0).cpu()
    ratio = torch.from_numpy(sd["dist"].abs().cpu().numpy() / np.float32(trunc))               # (on the host: a correctly rounded float32 division)
    expect = torch.where(found.cpu(), s * torch.minimum(ratio, torch.ones_like(s)), s)
    differ = expect != ts
    print(f"{S.grid_case_id(case)}: {int(differ.sum())} voxels differ from signed_distances; of them {int((differ & ((expect < 0) != (ts < 0))).sum())} in sign; "
          f"largest difference {float((expect - ts).abs().max()):.3e}")
    assert not bool(differ.any())
    assert torch.equal(found.cpu()[mask], hit[mask])


def test_exactly_half_counts_as_inside():
    v, f = S.half_octahedron()
    bvh = MB.build_bvh(v, f)
    mom = MS.node_moments(bvh)
    o = torch.zeros(1, 3)
    assert MS.winding_numbers(bvh, o, 0.0, mom).tolist() == [0.5]                # the premise: exactly 0.5 on the device too
    sd = MS.signed_distances(bvh, o, 0.0, moments=mom)
    assert float(sd["dist"][0]) < 0
    N, bound = S.HALF_GRID["N"], S.HALF_GRID["bound"]
    assert MS.voxel_centres(N, bound, DEV)[13].tolist() == [0.0, 0.0, 0.0]
    vol = MS._fill(bvh, mom, None, N, bound, 1.0, 0.0)
    assert float(vol.tsdf_sum.reshape(-1)[13]) < 0                               # `w > 0.5` would leave the voxel outside
    assert float(vol.tsdf_sum.reshape(-1)[13 - 9]) > 0                           # (0, 0, -1), below the open base: outside


def test_signed_distances_agree_with_winding_and_closest_points():
    v, f, bvh, mom, *_ = device_case("open")
    q = S.queries()
    sd = MS.signed_distances(bvh, q, 2.0, moments=mom)
    dist, face, uv = MQ.closest_points(bvh, q)
    w = MS.winding_numbers(bvh, q, 2.0, mom)
    assert torch.equal(sd["w"], w) and torch.equal(sd["face"], face) and torch.equal(sd["uv"], uv)
    assert torch.equal(sd["dist"].abs(), dist) and torch.equal(sd["dist"] < 0, w >= 0.5)
    assert bool((sd["dist"] < 0).any()) and bool((sd["dist"] > 0).any())
    short = MS.signed_distances(bvh, q, 2.0, max_dist=0.01, moments=mom)
    miss = short["face"] < 0
    assert bool(miss.any()) and torch.equal(short["dist"][miss], torch.where(w[miss] >= 0.5, -INF, INF))


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------
def closed_manifold(faces, num_verts):
    und, cnt, ssum = R.undirected_counts(faces)
    return bool((cnt == 2).all()) and not ssum.any(), num_verts - und.shape[0] + faces.shape[0]


@pytest.mark.parametrize("kind", ("closed", "open"))
def test_a_sphere_comes_out_closed(kind):
    v, f, bvh, mom, _, tree, mom_host, _, _ = device_case(kind)
    N, bound = S.E2E["N"], S.E2E["bound"]
    c = M.position_colors(v)
    _, open_in = MS.edge_counts(f, v.shape[0])
    assert (kind == "open") == (open_in > 0)
    ov, of, oc, stats = MS.solidify_mesh(v, f, c, resolution=N, bound=bound)
    assert stats["boundary_edges_before"] == open_in and stats["boundary_edges_after"] == 0 and stats["boundary_vertices_after"] == 0
    assert (stats["boundary_vertices_before"] > 0) == (kind == "open")
    ok, euler = closed_manifold(of.cpu().numpy(), ov.shape[0])
    assert ok and euler == 2 == stats["euler"]
    assert stats["volume"] == pytest.approx(R.signed_volume(ov.cpu().numpy(), of.cpu().numpy()), rel=1e-9) and 0.3 < stats["volume"] < 4.2 * 0.5 ** 3
    assert stats["bvh_rounds"] == bvh.rounds and stats["moment_rounds"] >= 2 and stats["mesh_distance"]["hausdorff"] < 0.25
    # the device's own volume through the restated extraction: the same faces, the same vertices
    trunc = S.grid_trunc(N, bound)
    vol = MS.mesh_to_volume(v, f, c, N, bound)
    assert vol.trunc == pytest.approx(trunc)
    host = dict(N=N, bound=bound, trunc=trunc, tsdf_sum=vol.tsdf_sum.reshape(-1).cpu(), weight=vol.weight.reshape(-1).cpu(),
                rgb_sum=vol.rgb_sum.reshape(3, -1).cpu(), rgb_weight=vol.rgb_weight.reshape(-1).cpu())
    hv, hf, hc, _, _ = R.extract(R.promoted(host))
    assert torch.equal(of.cpu().long(), hf) and float((ov.cpu().double() - hv).abs().max()) < 1e-6
    # Chamfer to the mesh of the fp64 volume, within 4x the float32 restatement's
    ref64 = R.extract(S.sdf_volume(tree, mom_host.double(), v, f, c, N, bound, trunc, S.GRID_BETA))[0]
    ref32 = R.extract(S.sdf_volume(tree, mom_host, v, f, c, N, bound, trunc, S.GRID_BETA, F32))[0]
    ch, bar = R.chamfer(ov.cpu(), ref64), 4 * R.chamfer(ref32, ref64)
    print(f"{kind}: {ov.shape[0]} vertices, {of.shape[0]} faces, Chamfer to the fp64 restatement's mesh {ch:.3e} (bar {bar:.3e})")
    record_parity(f"mesh_solid_e2e[{kind}]", {"chamfer": ch, "bar": bar, "vertices": int(ov.shape[0]), "faces": int(of.shape[0]), "volume": stats["volume"]})
    assert ch <= bar
    if kind == "open":                                    # the new cap sits about where the flat disc on the rim does: w = 0.5 there
        voxel = 2.0 * bound / N
        cap = S.cap_vertices(ov.cpu(), v, f, voxel)
        zlo, zhi = S.rim_heights()
        z = ov.cpu()[cap][:, 2]
        assert int(cap.sum()) > 10 and float(z.min()) >= zlo - 2 * voxel and float(z.max()) <= zhi + 2 * voxel


def test_the_reversed_sphere_is_empty_and_flip_restores_it():
    v, f = S.mesh("closed")
    c = M.position_colors(v)
    N, bound = S.E2E["N"], S.E2E["bound"]
    ov, of, oc, stats = MS.solidify_mesh(v, f[:, [0, 2, 1]], c, resolution=N, bound=bound)
    assert ov.shape[0] == 0 and of.shape[0] == 0 and stats["faces"] == 0 and stats["mesh_distance"] is None and stats["euler"] == 0
    a = MS.solidify_mesh(v, f, c, resolution=N, bound=bound)
    b = MS.solidify_mesh(v, f[:, [0, 2, 1]], c, resolution=N, bound=bound, flip=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and b[3]["flipped"]
    sm = MS.solidify_mesh(v, f, c, resolution=N, bound=bound, smooth=3)
    assert torch.equal(sm[1], a[1]) and not torch.equal(sm[0], a[0]) and sm[3]["smooth_iterations"] == 3


def test_script_end_to_end(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("solidify_mesh_script", os.path.join(ROOT, "scripts", "pub", "solidify_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    v, f = S.mesh("open")
    src, out, js = str(tmp_path / "open.ply"), str(tmp_path / "solid.ply"), str(tmp_path / "stats.json")
    G.save_mesh_ply(src, v, f, M.position_colors(v))
    mod.main(["--mesh", src, "-o", out, "--resolution", "24", "--bound", "0.7", "--smooth", "2", "--json", js, "--render_orbit", "2", "--reso", "64", "-w"])
    ov, of, oc = G.read_mesh_ply(out)
    ok, euler = closed_manifold(of, ov.shape[0])
    assert ok and euler == 2
    stats = json.load(open(js))
    assert stats["boundary_edges_before"] > 0 and stats["boundary_edges_after"] == 0 and stats["smooth_iterations"] == 2 and stats["faces"] == of.shape[0]
    frames = np.load(str(tmp_path / "solid_orbit" / "orbit.npy"))
    assert frames.shape == (2, 64, 64, 3) and frames.min() < 250 and os.path.exists(str(tmp_path / "solid_orbit" / "001.png"))
    # the empty result: a mesh wound inward, without --flip
    G.save_mesh_ply(src, v, f[:, [0, 2, 1]], M.position_colors(v))
    empty = str(tmp_path / "empty.ply")
    mod.main(["--mesh", src, "-o", empty, "--resolution", "24", "--bound", "0.7", "--render_orbit", "2", "--reso", "64"])
    assert "EMPTY" in capsys.readouterr().out and G.read_mesh_ply(empty)[1].shape[0] == 0
    assert json.load(open(str(tmp_path / "empty.json")))["mesh_distance"] is None
    mod.main(["--mesh", src, "-o", empty, "--resolution", "24", "--bound", "0.7", "--flip"])
    assert G.read_mesh_ply(empty)[1].shape[0] > 0
