"""The gfx950 mesh queries (csrc_recon/meshquery.hip, v3d_amd/recon/mesh_query.py, scripts/pub/mesh_distance.py and bake_ao.py) against the
torch restatement (tests/mesh_query_ref.py): the closest point against a brute force over all triangles, queries on box planes, ties and
limits, the midpoint samples, occlusion as an integer interval on every point, the frames of the atlas, the distance between two meshes,
the AO bake, guards around every output, and the scripts.

The bar for continuous outputs is that of tests/test_mesh_bake_gpu.py: the kernel may be off from the fp64 restatement by 4x what the
restatement's own float32 run is off, the float32 figure taken over the whole scene, once.  The closest point needs no exclusions: the
distance is held on every query, the returned (face, uv) must rebuild a point that close, and `face` itself is compared where the runner-up
is further than 1e-5.  Occlusion is held on every point: sure <= hits <= sure + marginal, where tests/test_mesh_query_cpu.py holds every
case to at most 2 % marginal rays."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_bake_ref as B
import mesh_query_ref as Q
import mesh_render_ref as M
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_bake as MB
from v3d_amd.recon import mesh_clean as MC
from v3d_amd.recon import mesh_decimate as MD
from v3d_amd.recon import mesh_query as MQ
from v3d_amd.recon import mesh_texture as MT

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
INF = float("inf")
GUARD = 4096


def _dev(t, dtype=None):
    return t.to(DEV, dtype) if dtype else t.to(DEV)


@functools.lru_cache(maxsize=None)
def scene_bvh(kind):
    v, f = (Q.occ_mesh(kind) if kind == "bumped" else M.mesh_scene(kind, 1)[:2])
    return MB.build_bvh(v, f)


class Guarded:
    """An output of n rows with GUARD sentinel elements before and after it"""

    def __init__(self, n, width, dtype, sentinel):
        self.n, self.width, self.sentinel = n, width, sentinel
        self.buf = torch.full((2 * GUARD + n * width,), sentinel, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def take(self):
        assert bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.n * self.width:] == self.sentinel).all()), "a guard was written"
        out = self.buf[GUARD:GUARD + self.n * self.width]
        return (out.reshape(self.n, self.width) if self.width > 1 else out).clone()


# ---- 1. the closest point -------------------------------------------------------------------------------------------------------------------
def check_points(v, f, p, got, r64, err32, label):
    """(a), (b), (c) of the module's docstring on host tensors; returns the figures"""
    dist, face, uv = got
    n = p.shape[0]
    assert dist.dtype == F32 and face.dtype == torch.int32 and tuple(uv.shape) == (n, 2)
    found = r64["face"] >= 0
    assert torch.equal(face >= 0, found)
    miss = face < 0
    assert bool((dist[miss] == INF).all()) and not uv[miss].any()
    derr = float((dist.double() - r64["dist"])[found].abs().max()) if bool(found.any()) else 0.0
    rebuilt = Q.rebuilt_distance(v, f, p, face, uv)
    rerr = float((rebuilt - r64["dist"])[found].abs().max()) if bool(found.any()) else 0.0
    assert float(uv.min()) >= -1e-6 and float(uv.sum(1).max()) <= 1 + 1e-6
    compared = found & (r64["runner"] - r64["dist"] > Q.FACE_GAP)
    share = float(compared.float().mean())
    print(f"{label}: N {n}: dist {derr:.3e}, rebuilt from (face, uv) {rerr:.3e} (float32 restatement {err32:.3e}); face compared on {share:.3f}")
    record_parity(f"mesh_query_points[{label}-{n}]", {"dist_max_abs": derr, "rebuilt_max_abs": rerr, "float32_restatement": err32, "face_compared_share": share})
    assert derr <= 4 * err32 and rerr <= 4 * err32
    assert torch.equal(face.long()[compared], r64["face"][compared])
    return derr, rerr, share


@pytest.mark.parametrize("n", Q.POINT_COUNTS)
@pytest.mark.parametrize("kind", ("sphere", "pair"))
def test_closest_point_matches_the_brute_force(kind, n):
    v, f, p, r64, r32 = Q.point_case(kind)
    err32 = float((r32["dist"].double() - r64["dist"]).abs().max())                  # over all 1100 queries of the scene
    bvh = scene_bvh(kind)
    got = [x.cpu() for x in MQ.closest_points(bvh, p[:n])]
    check_points(v, f, p[:n], got, {k: x[:n] for k, x in r64.items()}, err32, kind)
    at_vertex = r64["dist"][:n] == 0
    assert bool((got[0][at_vertex] == 0).all())
    again = [x.cpu() for x in MQ.closest_points(bvh, p[:n])]
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs differ"
    if n in (65, 1100):                                # guards around every output
        pd = _dev(p[:n]).contiguous()
        dist, face, uv = Guarded(n, 1, F32, -7.0), Guarded(n, 1, torch.int32, -7), Guarded(n, 2, F32, -7.0)
        lib = G.load_library()
        G._check(lib, lib.v3d_recon_bvh_closest_point(pd.data_ptr(), n, INF, *bvh._args(), dist.ptr, face.ptr, uv.ptr, G._stream()), "closest_point")
        assert all(torch.equal(a.cpu(), b) for a, b in zip((dist.take(), face.take(), uv.take()), got))


def test_queries_on_box_planes_of_nodes():
    """Queries exactly on the planes, edges and corners of nine nodes' boxes read back from the tree: bounds of exactly 0 on some axes"""
    kind = "sphere"
    v, f, _, r64_all, r32_all = Q.point_case(kind)
    bvh = scene_bvh(kind)
    F = f.shape[0]
    lo, hi = bvh.lo.cpu(), bvh.hi.cpu()
    nodes = [0, int(bvh.left[0]), int(bvh.right[0]), int(bvh.left[1]), F - 1 + 5, F - 1 + 100, 7, 50, 200]
    p = []
    for n in nodes:
        mid = 0.5 * (lo[n] + hi[n])
        for axis in range(3):
            for plane in (lo[n], hi[n]):
                q = mid.clone()
                q[axis] = plane[axis]
                p.append(q)                            # on a face of the box
                q = plane.clone()
                q[axis] = mid[axis]
                p.append(q)                            # on an edge of the box
        p += [lo[n].clone(), hi[n].clone()]            # at two corners
    p = torch.stack(p)
    err32 = float((r32_all["dist"].double() - r64_all["dist"]).abs().max())
    got = [x.cpu() for x in MQ.closest_points(bvh, p)]
    check_points(v, f, p, got, Q.closest_point(v, f, p), err32, "box_planes")


def test_deep_strip_degenerate_faces_ties_limits_and_single_faces():
    # the low-bit strip: a deep tree
    v, f = B.low_bit_strip()
    g = torch.Generator().manual_seed(5)
    step = 1.0 / 1024 / 8
    p = torch.cat([torch.rand(200, 3, generator=g) * torch.tensor([64 * step, 2 * step, 2 * step]) - torch.tensor([0.0, 0.5 * step, step]),
                   torch.rand(60, 3, generator=g) * 2.4 - 1.2])
    r64, r32 = Q.closest_point(v, f, p), Q.closest_point(v, f, p, dtype=F32)
    got = [x.cpu() for x in MQ.closest_points(MB.build_bvh(v, f), p)]
    check_points(v, f, p, got, r64, float((r32["dist"].double() - r64["dist"]).abs().max()), "low_bit_strip")
    assert len(set(got[1][:200].tolist())) > 40        # the strip's own triangles answer
    # the sphere with a zero-area face and a face with index V: never returned, and the other answers are the sphere's
    dv, df = B.degenerate_mesh()
    q = Q.queries("sphere")
    a = [x.cpu() for x in MQ.closest_points(MB.build_bvh(dv, df), q)]
    b = [x.cpu() for x in MQ.closest_points(scene_bvh("sphere"), q)]
    assert int(a[1].max()) < 320 and int(a[1].min()) >= 0 and all(torch.equal(x, y) for x, y in zip(a, b))
    # coincident triangles among equal Morton codes: the smaller index wins wherever the copies stand
    sv, sf = B.same_centroid_faces()
    tri = sv[sf[3]].double()
    inside = (0.5 * tri[0] + 0.3 * tri[1] + 0.2 * tri[2]).float()[None]
    for faces, want in ((torch.cat([sf[3:4]] * 9 + [sf[:3]]), 0), (torch.cat([sf[:3], sf[4:], sf[3:4], sf[3:4]]), 7), (torch.cat([sf, sf[3:4]]), 3)):
        dist, face, uv = (x.cpu() for x in MQ.closest_points(MB.build_bvh(sv, faces), inside))
        assert face.tolist() == [want] and float(dist) < 1e-6, (face.tolist(), want)
    # the exact case: every region, F = 1, the closed limit, just below it, inf, and a NaN query
    ev, ef, ep, ed = Q.exact_triangle()
    one = MB.build_bvh(ev, ef)
    dist, face, uv = (x.cpu() for x in MQ.closest_points(one, ep))
    assert face.tolist() == [0] * 7 and torch.equal(dist, ed.float())
    assert uv.tolist() == [[0, 0], [1, 0], [0.5, 0], [0, 1], [0, 0.5], [0.5, 0.5], [0.25, 0.25]]
    dist, face, _ = (x.cpu() for x in MQ.closest_points(one, ep, max_dist=2.0))
    assert face.tolist() == [0, -1, 0, -1, 0, -1, 0] and dist.tolist()[2] == 2.0 and dist.tolist()[1] == INF          # d == max_dist is found
    below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    dist, face, uv = (x.cpu() for x in MQ.closest_points(one, ep, max_dist=below))
    assert face.tolist() == [0, -1, -1, -1, -1, -1, -1] and dist.tolist()[2] == INF and not uv[1:].any()
    assert MQ.closest_points(one, ep, max_dist=0.0)[1].tolist() == [-1] * 7
    bad = torch.tensor([[0.0, float("nan"), 0.0], [INF, 0.0, 0.0], [1.0, 1.0, 2.0]])
    dist, face, uv = (x.cpu() for x in MQ.closest_points(one, bad))
    assert face.tolist() == [-1, -1, 0] and dist.tolist() == [INF, INF, 2.0] and not uv[:2].any()
    d0, f0, uv0 = MQ.closest_points(one, torch.zeros(0, 3))
    assert tuple(d0.shape) == (0,) and tuple(uv0.shape) == (0, 2) and d0.device.type == "cuda"


# ---- 2. the samples ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 16))
@pytest.mark.parametrize("kind", ("sphere", "ragged"))
def test_face_samples_match_the_restatement(kind, n):
    v, f = M.mesh_scene("sphere", 1)[:2]
    if kind == "ragged":                               # 37 faces: F n^2 ends in a partial block (at n = 16 a sample count is always whole blocks); one face with index V
        f = torch.cat([f[:36], torch.tensor([[0, v.shape[0], 2]])])
    F = f.shape[0]
    p64, w64, _ = Q.face_samples(v, f, n)
    p32, w32, _ = Q.face_samples(v, f, n, F32)
    vd, fd = _dev(v), _dev(f, torch.int32)
    pts, w = Guarded(F * n * n, 3, F32, -7.0), Guarded(F * n * n, 1, F32, -7.0)
    lib = G.load_library()
    G._check(lib, lib.v3d_recon_mesh_face_samples(vd.data_ptr(), v.shape[0], fd.data_ptr(), F, n, pts.ptr, w.ptr, G._stream()), "face_samples")
    pts, w = pts.take().cpu(), w.take().cpu()
    a, b = MQ.face_samples(v, f if kind == "sphere" else f[:36], n)
    assert torch.equal(a.cpu(), pts[:a.shape[0]]) and torch.equal(b.cpu(), w[:b.shape[0]])
    perr, perr32 = float((pts.double() - p64).abs().max()), float((p32.double() - p64).abs().max())
    werr, werr32 = float((w.double() - w64).abs().max()), float((w32.double() - w64).abs().max())
    print(f"{kind} n {n}: points {perr:.3e} (float32 restatement {perr32:.3e}), weights {werr:.3e} ({werr32:.3e})")
    record_parity(f"mesh_query_samples[{kind}-{n}]", {"points_max_abs": perr, "points_float32_restatement": perr32, "weights_max_abs": werr,
                                                      "weights_float32_restatement": werr32})
    assert perr <= 4 * perr32 and werr <= 4 * werr32
    area = float(w64.sum())
    serr, serr32 = abs(float(w.double().sum()) - area), abs(float(w32.double().sum()) - area)
    print(f"{kind} n {n}: the weights' sum {serr:.3e} from the area (float32 restatement {serr32:.3e})")
    # The sum is held to 4x the float32 restatement's PLUS 1e-7 of the area.  The restatement's figure alone is no bar here: it is a signed
    # sum of 320 n^2 rounding errors, and on the whole sphere they cancel to 3.8e-10, a ten-millionth of an ulp-sized share (1.2e-10 of the
    # area, where ONE rounding of a float is 6e-8): luck, as the ragged mesh shows, whose figure is ten times larger on a ninth of the faces.
    # Any other order of the same roundings (the kernel's fused multiply-adds) lands elsewhere inside the format's own band.  1e-7 of the
    # area is under two roundings (2 x 2^-24 = 1.2e-7) of the total and eight times below what the per-weight bar above already allows
    # for the sum; every single weight is held to the plain 4x bar.
    assert serr <= 4 * serr32 + 1e-7 * area
    if kind == "ragged":
        assert not pts[36 * n * n:].any() and not w[36 * n * n:].any() and bool((w[:36 * n * n] > 0).all())


# ---- 3. occlusion -----------------------------------------------------------------------------------------------------------------------------
def check_hits(hits, ref, K, label):
    """sure <= hits <= sure + marginal on every point, and the cap that keeps the interval from hiding a failure: at most 2 % of the rays
    compared here are marginal (tests/test_mesh_query_cpu.py holds the same on the CPU for every case)"""
    hits = hits.cpu().long()
    lo, hi = ref["sure"], ref["sure"] + ref["marginal"]
    assert int(ref["marginal"].sum()) <= Q.MARGINAL_MAX * K * hits.shape[0], (label, int(ref["marginal"].sum()), K * hits.shape[0])
    wrong = (hits < lo) | (hits > hi)
    print(f"{label}: hits {int(hits.min())} .. {int(hits.max())}, {int(ref['marginal'].sum())} marginal rays, {int((hits != ref['hits']).sum())} points off the "
          f"restatement's own count")
    assert not bool(wrong.any()), (hits[wrong].tolist(), lo[wrong].tolist(), hi[wrong].tolist())


@pytest.mark.parametrize("case", Q.OCC_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_occlusion_is_inside_the_interval_on_every_point(case):
    name, K, radius = case
    first = case == Q.OCC_CASES[0]
    counts = Q.OCC_COUNTS if first else (Q.OCC_SMALL,)
    ref = Q.occ_case(name, K, radius, max(counts))
    p, nrm = Q.occ_points(name)
    bvh = scene_bvh(name)
    for n in counts:
        hits = MQ.occlusion(bvh, p[:n], nrm[:n], K, radius, Q.AO_BIAS)
        assert hits.dtype == torch.int32 and tuple(hits.shape) == (n,)
        check_hits(hits, {k: x[:n] for k, x in ref.items()}, K, f"{name} K {K} radius {radius} N {n}")
        assert torch.equal(hits, MQ.occlusion(bvh, p[:n], nrm[:n], K, radius, Q.AO_BIAS)), "two runs differ"
    record_parity(f"mesh_query_occlusion[{name}-{K}-{radius}]", {"points": max(counts), "marginal_rays": int(ref["marginal"].sum()),
                                                               "occluded_share": float(ref["sure"].sum()) / (max(counts) * K)})
    if first:
        n = 65
        sp, sn, sK, sr, sb, seed = Q.extra_occ_inputs("seed")
        assert (sK, sr, sb) == (K, radius, Q.AO_BIAS) and torch.equal(sp, p[:n]) and torch.equal(sn, nrm[:n])
        other = MQ.occlusion(bvh, sp, sn, sK, sr, sb, seed=seed)
        assert not torch.equal(other, hits[:n])
        check_hits(other, Q.extra_occ_case("seed")[0], K, f"seed {seed}")
        pd, nd = _dev(p[:n]).contiguous(), _dev(nrm[:n]).contiguous()
        out = Guarded(n, 1, torch.int32, -7)
        lib = G.load_library()
        G._check(lib, lib.v3d_recon_bvh_occlusion(pd.data_ptr(), nd.data_ptr(), n, K, radius, Q.AO_BIAS, 0, *bvh._args(), out.ptr, G._stream()), "occlusion")
        assert torch.equal(out.take(), hits[:n])


def test_occlusion_of_points_that_are_not_valid_lifted_points_and_known_scenes():
    bvh = scene_bvh("pair")
    p, nrm, K, radius, bias, seed = Q.extra_occ_inputs("invalid")
    ref, _ = Q.extra_occ_case("invalid")
    hits = MQ.occlusion(bvh, p, nrm, K, radius, bias, seed=seed).cpu()
    assert (~ref["valid"]).nonzero().reshape(-1).tolist() == [3, 10, 20, 30, 40]
    assert bool((hits[~ref["valid"]] == -1).all())
    check_hits(hits[ref["valid"]], {k: x[ref["valid"]] for k, x in ref.items()}, K, "with invalid points")
    # bias = 0, from points lifted off the surface
    lp, ln, K, radius, bias, seed = Q.extra_occ_inputs("bias0")
    assert bias == 0.0
    check_hits(MQ.occlusion(bvh, lp, ln, K, radius, bias, seed=seed), Q.extra_occ_case("bias0")[0], K, "bias 0")
    # F = 1: a large triangle over the point, and beside it
    tv, tf = torch.tensor([[-50.0, -50.0, 1.0], [50.0, -50.0, 1.0], [0.0, 80.0, 1.0]]), torch.tensor([[0, 1, 2]])
    up = torch.tensor([[0.0, 0.0, 1.0]])
    one = MB.build_bvh(tv, tf)
    origin = torch.tensor([[0.1, 0.2, 0.0]])
    assert MQ.occlusion(one, origin, up, 200, 30.0, 0.0).tolist() == Q.occlusion(tv, tf, origin, up, 200, 30.0, 0.0)["hits"].tolist()
    assert MQ.occlusion(one, origin, up, 200, 0.5, 0.0).tolist() == [0]
    assert MQ.occlusion(one, origin, -up, 200, 30.0, 0.0).tolist() == [0]
    # the quad and the cube of tests/test_mesh_query_cpu.py: exactly 0, exactly K
    qv, qf = Q.quad(100.0)
    assert MQ.occlusion(MB.build_bvh(qv, qf), torch.tensor([[0.3, -0.2, 0.1]]), up, 64, 50.0, 0.0).tolist() == [0]
    cv, cf = Q.cube(1.0)
    centre, tilt = torch.tensor([[0.01, 0.02, -0.015]]), torch.tensor([[0.3, 0.5, 0.8]])
    box = MB.build_bvh(cv, cf)
    for K in (1, 64, 65, 1024):
        assert MQ.occlusion(box, centre, tilt, K, 10.0, 0.0).tolist() == [K]
        assert MQ.occlusion(box, centre, tilt, K, 0.45, 0.0).tolist() == [0]
    assert tuple(MQ.occlusion(box, torch.zeros(0, 3), torch.zeros(0, 3)).shape) == (0,)


# ---- 4. the frames of the atlas ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tex", B.BAKE_SIZES)
def test_texel_frames_are_the_normal_bakes(tex):
    lv, lf, hv, hf, md = B.bake_scene("nested")
    lvd, lfd, hvd, hfd = _dev(lv), _dev(lf, torch.int32), _dev(hv), _dev(hf, torch.int32)
    ln = MC.vertex_normals(lvd, lfd)
    owner, P, n = MQ.texel_frames(lvd, lfd, ln, tex)
    bake_owner = MB.bake_texels(lvd, lfd, ln, MB.build_bvh(hvd, hfd), MC.vertex_normals(hvd, hfd), tex, md)[0]
    assert torch.equal(owner, bake_owner)
    o64, cast, P64, n64 = Q.texel_frames(lv, lf, ln.cpu(), tex)
    _, _, P32, n32 = Q.texel_frames(lv, lf, ln.cpu(), tex, F32)
    owner, P, n = owner.cpu().long(), P.cpu(), n.cpu()
    assert torch.equal(owner, o64) and torch.equal(cast, owner >= 0)
    assert bool(torch.isnan(P[~cast]).all()) and bool((n[~cast] == torch.tensor([0.0, 0.0, 1.0])).all())
    perr, perr32 = float((P.double() - P64)[cast].abs().max()), float((P32.double() - P64)[cast].abs().max())
    nerr, nerr32 = float((n.double() - n64)[cast].abs().max()), float((n32.double() - n64)[cast].abs().max())
    print(f"R {tex}: P {perr:.3e} (float32 restatement {perr32:.3e}), n {nerr:.3e} ({nerr32:.3e})")
    record_parity(f"mesh_query_frames[{tex}]", {"position_max_abs": perr, "position_float32_restatement": perr32, "normal_max_abs": nerr,
                                                "normal_float32_restatement": nerr32})
    assert perr <= 4 * perr32 and nerr <= 4 * nerr32


# ---- 5. the distance --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decimated_pair():
    """The project's own chain: the extracted 24^3 sphere and its decimation to a quarter of its faces, on the host"""
    ref = B.R.sphere_volume(24, 1.0, 0.5)
    N = ref["N"]
    f32 = lambda t, *s: t.float().reshape(*s).contiguous().to(DEV)  # noqa: E731
    vol = G.TsdfVolume(N, ref["bound"], ref["trunc"], f32(ref["tsdf_sum"], N, N, N), f32(ref["weight"], N, N, N), f32(ref["rgb_sum"], 3, N, N, N),
                       f32(ref["rgb_weight"], N, N, N))
    v, f, _ = G.extract_mesh(vol)
    vd, fd, _, _ = MD.decimate_mesh(v, f, None, f.shape[0] // 4)
    return vd.cpu(), fd.cpu().long(), v.cpu(), f.cpu().long()


@pytest.mark.parametrize("name", ("spheres", "decimated"))
def test_mesh_distance_matches_the_restatement(name):
    av, af, bv, bf = Q.distance_pair() if name == "spheres" else decimated_pair()
    d = MQ.mesh_distance(av, af, bv, bf, subdivide=2)
    r64, r32 = Q.mesh_distance(av, af, bv, bf, 2), Q.mesh_distance(av, af, bv, bf, 2, F32)
    got, want = Q.distance_figures(d), Q.distance_figures(r64)
    names = ("a_to_b mean", "a_to_b rms", "a_to_b max", "b_to_a mean", "b_to_a rms", "b_to_a max", "hausdorff", "chamfer")
    # Every figure is a maximum or a weighted mean of the queried points' distances, so it is off by no more than the worst of them: the
    # float32 figure is the restatement's worst distance over all points of both directions
    err32 = max(float((r32[k]["dists"] - r64[k]["dists"]).abs().max()) for k in ("a_to_b", "b_to_a"))
    # ... and to 4x what the float32 restatement's own figures are off, the largest over the eight figures of the scene
    fmt = Q.distance_figures(r32)
    fig32 = max(abs(a - b) for a, b in zip(fmt, want))
    for i, nm in enumerate(names):
        print(f"{name}: {nm} {got[i]:.6e} (restatement {want[i]:.6e}, off {abs(got[i] - want[i]):.3e}; float32 restatement's figure off "
              f"{abs(fmt[i] - want[i]):.3e}, its worst figure {fig32:.3e}, its worst distance {err32:.3e})")
    for i, nm in enumerate(names):
        assert abs(got[i] - want[i]) <= 4 * err32 and abs(got[i] - want[i]) <= 4 * fig32, nm
    record_parity(f"mesh_query_distance[{name}]", {"hausdorff": d["hausdorff"], "chamfer": d["chamfer"], "hausdorff_restatement": r64["hausdorff"],
                                                   "faces_a": int(af.shape[0]), "faces_b": int(bf.shape[0]), "samples": d["samples"],
                                                   "float32_restatement": err32, "float32_restatement_figures": fig32})
    assert d["a_to_b"]["max"] >= r64["a_to_b"]["vertex_max"] - 4 * err32 and d["b_to_a"]["max"] >= r64["b_to_a"]["vertex_max"] - 4 * err32
    bvh_b = MB.build_bvh(bv, bf)
    assert d["a_to_b"]["max"] >= float(MQ.closest_points(bvh_b, av)[0].max())            # the maximum is >= every vertex's distance
    assert d["hausdorff"] == max(d["a_to_b"]["max"], d["b_to_a"]["max"]) and d["chamfer"] == 0.5 * (d["a_to_b"]["mean"] + d["b_to_a"]["mean"])
    assert d["samples"] == 4 * (af.shape[0] + bf.shape[0]) + av.shape[0] + bv.shape[0]
    assert abs(d["relative"]["hausdorff"] * d["diagonal"] - d["hausdorff"]) < 1e-12 and abs(d["diagonal"] - r64["diagonal"]) < 1e-6
    same = MQ.mesh_distance(bv, bf, bv, bf, subdivide=1)
    assert same["hausdorff"] <= 4 * err32


# ---- 6. the AO bake ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tex", B.BAKE_SIZES)
def test_ambient_occlusion_bake(tex):
    lv, lf, hv, hf, md, radius = Q.ao_scene()
    K = 32
    ao, stats = MQ.bake_ambient_occlusion(lv, lf, hv, hf, tex_size=tex, samples=K, radius=radius, bias=Q.AO_BIAS, max_dist=md)
    again, _ = MQ.bake_ambient_occlusion(lv, lf, hv, hf, tex_size=tex, samples=K, radius=radius, bias=Q.AO_BIAS, max_dist=md)
    assert torch.equal(ao, again), "two runs differ"
    ao = ao.cpu()
    assert ao.dtype == F32 and tuple(ao.shape) == (tex * tex,)
    lvd, lfd, hvd, hfd = _dev(lv), _dev(lf, torch.int32), _dev(hv), _dev(hf, torch.int32)
    ln, hn = MC.vertex_normals(lvd, lfd).cpu(), MC.vertex_normals(hvd, hfd).cpu()      # the restatement is fed the kernel's own vertex normals
    ref = Q.bake_ao(lv, lf, ln, hv, hf, hn, tex, md, K, radius, Q.AO_BIAS)
    cast, rows = ref["cast"], ref["cast"] & ref["keep"]
    assert bool((ao[~cast] == 1.0).all())                                              # unowned: exactly 1
    hits = torch.round((1.0 - ao.double()) * K).long()
    assert float(((1.0 - hits.double() / K).float() - ao).abs().max()) == 0
    check_hits(hits[rows], {k: ref[k][rows] for k in ("sure", "marginal", "hits")}, K, f"ao R {tex}")
    assert stats["owned"] == int(cast.sum()) and stats["rays"] == K * int(cast.sum()) and stats["samples"] == K and stats["tex_size"] == tex
    assert abs(stats["mean_ao"] - float(ao[cast].double().mean())) < 1e-9 and stats["min_ao"] == float(ao[cast].min())
    assert stats["fully_open"] == int((ao[cast] == 1).sum()) and stats["radius"] == radius and stats["bias"] == Q.AO_BIAS
    sign = Q.bump_sign(ref["points"][rows])
    dimple, bump = float(ao[rows][sign < -0.3].double().mean()), float(ao[rows][sign > 0.3].double().mean())
    print(f"R {tex}: {int(rows.sum())} of {int(cast.sum())} texels compared; mean ao {stats['mean_ao']:.4f}, over dimples {dimple:.4f}, over bumps {bump:.4f}")
    record_parity(f"mesh_query_ao[{tex}]", {"mean_ao": stats["mean_ao"], "dimples": dimple, "bumps": bump, "compared_share": float(rows.sum()) / float(cast.sum())})
    assert dimple < bump
    # the defaults are shares of the high mesh's diagonal
    _, st = MQ.bake_ambient_occlusion(lv, lf, hv, hf, tex_size=tex, samples=1)
    diag = float((hv.max(0).values - hv.min(0).values).norm())
    assert abs(st["radius"] - 0.1 * diag) < 1e-6 and abs(st["bias"] - 1e-4 * diag) < 1e-9 and abs(st["max_dist"] - 0.05 * diag) < 1e-6


# ---- 7. the scripts ---------------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_scripts_end_to_end(tmp_path, capsys):
    lv, lf, hv, hf, md, radius = Q.ao_scene()
    low, high = str(tmp_path / "low.ply"), str(tmp_path / "high.ply")
    G.save_mesh_ply(low, lv, lf, M.position_colors(lv))
    G.save_mesh_ply(high, hv, hf, M.position_colors(hv))
    _entry("mesh_distance").main(["--mesh", low, "--reference", high, "--subdivide", "2", "--json", str(tmp_path / "d.json")])
    out = capsys.readouterr().out
    assert "Hausdorff" in out and "back:" in out and "% of the diagonal" in out
    d = json.load(open(tmp_path / "d.json"))
    want = MQ.mesh_distance(lv, lf, hv, hf, subdivide=2)
    assert d["hausdorff"] == want["hausdorff"] and d["a_to_b"] == want["a_to_b"] and d["b_to_a"] == want["b_to_a"] and d["mesh_faces"] == 320
    assert d["relative"]["hausdorff"] == want["relative"]["hausdorff"] and d["reference_faces"] == 1280 and d["subdivide"] == 2
    # bake_ao.py on an OBJ written by bake_normals.py: all three maps
    R = 64
    nm = str(tmp_path / "nm.obj")
    _entry("bake_normals").main(["--mesh", low, "--high", high, "-o", nm, "--texture_resolution", str(R), "--views", "0", "--max_dist", str(md)])
    os.makedirs(tmp_path / "ao")
    ao_obj = str(tmp_path / "ao" / "ao.obj")
    _entry("bake_ao").main(["--mesh", nm, "--high", high, "-o", ao_obj, "--samples", "32", "--ao_radius", str(radius), "--ao_bias", str(Q.AO_BIAS),
                            "--max_dist", str(md), "--texture_resolution", "512", "--render_orbit", "2", "--reso", "64", "--elevation", "15", "-w"])
    out = capsys.readouterr().out
    assert "fully open" in out and "turntable" in out
    assert sorted(os.listdir(tmp_path / "ao")) == ["ao.mtl", "ao.obj", "ao.png", "ao_ao.json", "ao_ao.png", "ao_ao_orbit", "ao_normal.png"]
    assert sorted(os.listdir(tmp_path / "ao" / "ao_ao_orbit")) == ["000.png", "001.png", "orbit.npy"]
    assert open(tmp_path / "ao" / "ao.mtl").read().endswith("map_Kd ao.png\nnorm ao_normal.png\nmap_Ka ao_ao.png\n")
    assert open(tmp_path / "ao" / "ao_normal.png", "rb").read() == open(tmp_path / "nm_normal.png", "rb").read()
    assert open(tmp_path / "ao" / "ao.png", "rb").read() == open(tmp_path / "nm.png", "rb").read()                  # the texture and its R are kept
    stats = json.load(open(tmp_path / "ao" / "ao_ao.json"))
    assert {"owned", "mean_ao", "min_ao", "fully_open", "samples", "radius", "bias", "rays", "bvh_rounds", "seconds"} <= set(stats)
    assert stats["samples"] == 32 and stats["tex_size"] == R and stats["normal_map_kept"] is True
    from PIL import Image
    img = np.asarray(Image.open(tmp_path / "ao" / "ao_ao.png"))
    ao, _ = MQ.bake_ambient_occlusion(lv, lf, hv, hf, tex_size=R, samples=32, radius=radius, bias=Q.AO_BIAS, max_dist=md)
    assert img.shape == (R, R) and np.array_equal(img.reshape(-1), np.floor(np.clip(ao.cpu().numpy(), 0, 1) * 255.0 + 0.5).astype(np.uint8))
    rv, rf, _, rtex = MT.read_textured_obj(ao_obj)
    assert np.array_equal(rf, lf.numpy()) and rtex.shape == (R * R, 3)
    frames = np.load(tmp_path / "ao" / "ao_ao_orbit" / "orbit.npy")
    assert frames.shape == (2, 64, 64, 3) and int((frames != 255).any(-1).sum()) > 800
