"""The mesh queries of libv3d_recon.so (csrc_recon/meshquery.hip, v3d_amd/recon/mesh_query.py, scripts/pub/mesh_distance.py and bake_ao.py)
without a GPU: header, ctypes table and exports agree, bad arguments are refused before any launch, the torch restatement
(tests/mesh_query_ref.py) is honest on cases with known answers, the OBJ writer with and without an AO map, the scripts' options, the host
API's refusals and empty cases, and the premises of the cases of tests/test_mesh_query_gpu.py on the restatement alone."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_bake_ref as B
import mesh_clean_ref as C
import mesh_query_ref as Q
import mesh_render_ref as M
import mesh_texture_ref as TX
from v3d_amd.recon import mesh_query as MQ                                      # (without the feature: the import fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_ENTRIES = {"v3d_recon_bvh_closest_point", "v3d_recon_mesh_face_samples", "v3d_recon_bvh_occlusion", "v3d_recon_tex_texel_frames"}
F64, F32 = torch.float64, torch.float32
INF = float("inf")


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
    assert QUERY_ENTRIES <= declared and declared == set(geometry.SIGNATURES)
    for name in QUERY_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert int(re.search(r"#define V3D_RECON_ABI_VERSION (\d+)", hdr).group(1)) == 1
    assert "Mesh queries" in hdr and "THE CLOSEST POINT OF A TRIANGLE" in hdr and "DIRECTION k OF POINT i" in hdr
    assert int(re.search(r"#define V3D_RECON_SAMPLES_MAX_SUBDIVIDE (\d+)", hdr).group(1)) == MQ.MAX_SUBDIVIDE == 16
    assert int(re.search(r"#define V3D_RECON_OCCLUSION_MAX_SAMPLES (\d+)", hdr).group(1)) == MQ.MAX_SAMPLES == 1024
    csrc = os.path.join(ROOT, "v3d_amd", "csrc_recon")
    src = open(os.path.join(csrc, "meshquery.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")
    # the walk is shared, not copied: one definition, in the header both sources include
    walk, bvh = open(os.path.join(csrc, "bvh_walk.h")).read(), open(os.path.join(csrc, "meshbvh.hip")).read()
    for name in ("struct Tree", "struct Ray", "struct Hit", "void slab(", "bool enters(", "void hit_triangle(", "Hit closest_hit(", "bool unit(", "bool vert_ok("):
        assert name in walk and name not in bvh and name not in src, name
    assert '#include "bvh_walk.h"' in bvh and '#include "bvh_walk.h"' in src


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

    cp = calls(lib.v3d_recon_bvh_closest_point, ("points", "N", "md") + tree + ("dist", "face", "uv", "stream"),
               points=p, N=100, md=INF, dist=p, face=p, uv=p, stream=None, **tree_defaults)
    for k in ("points", "dist", "face", "uv"):
        assert cp(**{k: None}) == -1 and "v3d_recon_bvh_closest_point" in err() and "null" in err(), k
    tree_refusals(cp, "v3d_recon_bvh_closest_point")
    assert cp(N=0) == -1 and "num_points" in err()
    assert cp(N=-1) == -1 and "num_points" in err()
    assert cp(md=-1.0) == -1 and "max_dist" in err()
    assert cp(md=float("nan")) == -1 and "max_dist" in err()
    fs = calls(lib.v3d_recon_mesh_face_samples, ("verts", "V", "faces", "F", "n", "points", "weights", "stream"),
               verts=p, V=162, faces=p, F=320, n=2, points=p, weights=p, stream=None)
    for k in ("verts", "faces", "points", "weights"):
        assert fs(**{k: None}) == -1 and "v3d_recon_mesh_face_samples" in err() and "null" in err(), k
    assert fs(V=0) == -1 and "num_verts" in err()
    assert fs(F=0) == -1 and "num_faces" in err()
    assert fs(n=0) == -1 and "subdivide 0" in err() and "16" in err()
    assert fs(n=17) == -1 and "subdivide 17" in err()
    assert fs(F=2 ** 31 - 1, n=2) == -1 and "int32" in err()
    assert fs(F=(2 ** 31 - 1) // 256 + 1, n=16) == -1 and "int32" in err()
    oc = calls(lib.v3d_recon_bvh_occlusion, ("points", "normals", "N", "K", "radius", "bias", "seed") + tree + ("hits", "stream"),
               points=p, normals=p, N=100, K=64, radius=0.1, bias=1e-4, seed=0, hits=p, stream=None, **tree_defaults)
    for k in ("points", "normals", "hits"):
        assert oc(**{k: None}) == -1 and "v3d_recon_bvh_occlusion" in err() and "null" in err(), k
    tree_refusals(oc, "v3d_recon_bvh_occlusion")
    assert oc(N=0) == -1 and "num_points" in err()
    assert oc(K=0) == -1 and "num_samples 0" in err() and "1024" in err()
    assert oc(K=1025) == -1 and "num_samples 1025" in err()
    for bad in (0.0, -1.0, INF, float("nan")):
        assert oc(radius=bad) == -1 and "radius" in err(), bad
    for bad in (-1e-3, INF, float("nan")):
        assert oc(bias=bad) == -1 and "bias" in err(), bad
    tf = calls(lib.v3d_recon_tex_texel_frames, ("verts", "V", "faces", "F", "normals", "R", "owner", "P", "n", "stream"),
               verts=p, V=162, faces=p, F=320, normals=p, R=64, owner=p, P=p, n=p, stream=None)
    for k in ("verts", "faces", "normals", "owner", "P", "n"):
        assert tf(**{k: None}) == -1 and "v3d_recon_tex_texel_frames" in err() and "null" in err(), k
    assert tf(V=0) == -1 and "num_verts" in err()
    assert tf(F=0) == -1 and "num_faces" in err()
    assert tf(R=0) == -1 and "tex_size 0" in err()
    assert tf(R=4097) == -1 and "tex_size 4097" in err()
    assert tf(R=32) == -1 and "too small" in err()


# ---- the restatement is honest ----------------------------------------------------------------------------------------------------------------
def test_closest_point_takes_every_region_and_is_exact_where_float32_is():
    v, f, p, d = Q.exact_triangle()
    r64, r32 = Q.closest_point(v, f, p), Q.closest_point(v, f, p, dtype=F32)
    assert r64["region"].tolist() == r32["region"].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert r64["face"].tolist() == [0] * 7
    assert torch.allclose(r64["dist"], d, rtol=0, atol=1e-15)
    assert torch.equal(r64["uv"].float(), r32["uv"]) and torch.equal(r64["dist"].float(), r32["dist"])
    assert r64["uv"].tolist() == [[0, 0], [1, 0], [0.5, 0], [0, 1], [0, 0.5], [0.5, 0.5], [0.25, 0.25]]
    # the closed limit, and a value just below the distance
    assert Q.closest_point(v, f, p[2:3], max_dist=2.0)["face"].tolist() == [0]
    assert Q.closest_point(v, f, p[2:3], max_dist=2.0, dtype=F32)["face"].tolist() == [0]
    below = Q.closest_point(v, f, p[2:3], max_dist=float(np.nextafter(np.float32(2.0), np.float32(0.0))))
    assert below["face"].tolist() == [-1] and below["dist"].tolist() == [INF] and below["uv"].tolist() == [[0, 0]]
    nan = Q.closest_point(v, f, torch.tensor([[0.0, float("nan"), 0.0]]))
    assert nan["face"].tolist() == [-1] and nan["dist"].tolist() == [INF]


def test_closest_point_of_an_icosphere_from_twice_its_radius():
    r = 0.5
    v, f = M.icosphere(2, r)
    vd = v.double()
    edge = float((vd[f[:, 0]] - vd[f[:, 1]]).norm(dim=1).max())
    circum = edge / math.sqrt(3.0)                           # no further from a face's centre than its circumradius (about: near-equilateral)
    sagitta = r - math.sqrt(r * r - (1.1 * circum) ** 2)
    g = torch.Generator().manual_seed(0)
    p = torch.nn.functional.normalize(torch.randn(500, 3, generator=g, dtype=F64), dim=1) * 2 * r
    d = Q.closest_point(v, f, p)["dist"]
    assert float(d.min()) >= r - 1e-7 and float(d.max()) <= r + sagitta
    assert float(d.max()) > r + 0.2 * sagitta                # and the bound is not idle


def test_skipped_faces_and_the_tie_rule():
    v, f = B.degenerate_mesh()
    p = torch.cat([v[:40], v[:40] * 1.3])
    r = Q.closest_point(v, f, p)
    assert int(r["face"].max()) < 320 and int(r["face"].min()) >= 0
    assert bool((r["dist"][:40] == 0).all())
    # coincident triangles: the smaller index
    tv = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    r = Q.closest_point(tv, torch.tensor([[0, 1, 2], [1, 2, 0], [0, 1, 2]]), torch.tensor([[0.25, 0.25, 1.0]]))
    assert r["face"].tolist() == [0] and r["runner"].tolist() == [1.0]


@pytest.mark.parametrize("n", (1, 2, 3, 16))
def test_face_samples_cover_their_faces(n):
    v, f = M.mesh_scene("sphere", 1)[:2]
    pts, w, b = Q.face_samples(v, f, n)
    assert tuple(pts.shape) == (320 * n * n, 3) and len(Q.sample_order(n)) == n * n
    vd = v.double()
    area = 0.5 * torch.linalg.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]]).norm(dim=1)
    assert abs(float(w.sum()) - float(area.sum())) < 1e-12
    assert bool((b > 0).all()) and bool((b.sum(1) < 1).all())                    # strictly inside
    assert abs(float(b[:, 0].mean()) - 1 / 3) < 1e-7 and abs(float(b[:, 1].mean()) - 1 / 3) < 1e-7         # the centroids' centroid is the face's
    r = Q.closest_point(v, f, pts[::7])
    assert float(r["dist"].max()) < 1e-12
    # a face with an index outside the vertices
    pts, w, _ = Q.face_samples(v, torch.tensor([[0, 1, 2], [0, v.shape[0], 2]]), n)
    assert not pts[n * n:].any() and not w[n * n:].any() and bool((w[:n * n] > 0).all())


def test_directions_are_unit_cosine_weighted_and_above_the_surface():
    g = torch.Generator().manual_seed(2)
    nrm = torch.randn(50, 3, generator=g) * 3.0
    nrm[0] = torch.tensor([0.0, 0.0, -2.0])                  # the frame's other branch, at its pole
    nrm[1] = torch.tensor([0.0, 0.0, 1.0])
    d, n, z = Q.sample_directions(nrm, 1024, seed=7)
    assert float((d.norm(dim=2) - 1).abs().max()) < 1e-12 and float((n.norm(dim=1) - 1).abs().max()) < 1e-12
    cosine = (d * n[:, None, :]).sum(2)
    assert float(cosine.min()) > 0 and float((cosine - z[None]).abs().max()) < 1e-12
    assert abs(float(z.mean()) - 2 / 3) < 1e-3
    d32, _, _ = Q.sample_directions(nrm, 1024, seed=7, dtype=F32)
    assert float((d32.double() - d).abs().max()) < 2e-6      # the same angle to 2^-24 of a turn: 2 pi 2^-24 = 4e-7, and the format's rounding
    other, _, _ = Q.sample_directions(nrm, 1024, seed=8)
    assert float((other - d).abs().max()) > 0.1
    # the hash: 32-bit words, different per point
    h = Q.point_hash(np.arange(1000), 0)
    assert h.max() < 2 ** 32 and len(set(h.tolist())) == 1000


def test_occlusion_of_a_quad_a_cube_and_a_wall():
    up = torch.tensor([[0.0, 0.0, 1.0]])
    v, f = Q.quad(100.0)
    o = Q.occlusion(v, f, torch.tensor([[0.3, -0.2, 0.1]]), up, 64, 50.0, 0.0)
    assert o["sure"].tolist() == o["marginal"].tolist() == o["hits"].tolist() == [0]
    v, f = Q.cube(1.0)
    centre = torch.tensor([[0.01, 0.02, -0.015]])            # (off the diagonals: no ray through an edge)
    o = Q.occlusion(v, f, centre, torch.tensor([[0.3, 0.5, 0.8]]), 64, 10.0, 0.0)
    assert o["sure"].tolist() == o["hits"].tolist() == [64] and o["marginal"].tolist() == [0]
    o = Q.occlusion(v, f, centre, torch.tensor([[0.3, 0.5, 0.8]]), 64, 0.45, 0.0)
    assert o["sure"].tolist() == o["hits"].tolist() == o["marginal"].tolist() == [0]
    assert Q.occlusion(v, f, centre, torch.zeros(1, 3), 64, 10.0, 0.0)["hits"].tolist() == [-1]
    assert Q.occlusion(v, f, torch.tensor([[INF, 0.0, 0.0]]), up, 64, 10.0, 0.0)["hits"].tolist() == [-1]
    # a wall of height h, a away: the form factor of a strip seen from the floor, 1/2 (1 - a / sqrt(a^2 + h^2))
    L, h = 1000.0, 1.0
    wall = torch.tensor([[1.0, -L, 0.0], [1.0, L, 0.0], [1.0, L, h], [1.0, -L, h]])
    wf = torch.tensor([[0, 1, 2], [0, 2, 3]])
    worst = 0.0
    for a in (0.5, 1.0, 2.0):
        pts = torch.tensor([[1.0 - a, 0.1 * k, 0.0] for k in range(8)])
        o = Q.occlusion(wall, wf, pts, up.expand(8, 3), 1024, 900.0, 0.0)
        got = o["hits"].double() / 1024
        want = 0.5 * (1 - a / math.sqrt(a * a + h * h))
        worst = max(worst, float((got - want).abs().max()))
        # WALL_DEVIATION: the restatement's own largest fp64 deviation over these 24 points at K = 1024, measured once; the tolerance is twice that
        assert float((got - want).abs().max()) <= 2 * WALL_DEVIATION, (a, got.tolist(), want)
    print(f"wall: largest deviation {worst:.3e}")


WALL_DEVIATION = 3.9e-3          # measured: 3.880e-03 (a = 0.5, the eighth point)


def test_the_saving_of_the_restatement_changes_no_count():
    v, f = Q.occ_mesh("pair")
    p, n = Q.occ_points("pair")
    a = Q.occlusion(v, f, p[:40], n[:40], 65, 0.1, Q.AO_BIAS)
    b = Q.occlusion(v, f, p[:40], n[:40], 65, 0.1, Q.AO_BIAS, cull=False)
    for k in ("sure", "marginal", "hits"):
        assert torch.equal(a[k], b[k]), k


def test_mesh_distance_of_a_mesh_to_itself_and_of_two_spheres():
    v, f = M.icosphere(3, 0.5)
    d = Q.mesh_distance(v, f, v, f, 2)
    assert max(Q.distance_figures(d)) < 1e-12
    e = 0.02
    v2, f2 = M.icosphere(3, 0.5 + e)
    vd = v.double()
    edge = float((vd[f[:, 0]] - vd[f[:, 1]]).norm(dim=1).max()) * (0.5 + e) / 0.5
    sagitta = (0.5 + e) - math.sqrt((0.5 + e) ** 2 - (1.1 * edge / math.sqrt(3.0)) ** 2)
    d = Q.mesh_distance(v, f, v2, f2, 2)
    for x in Q.distance_figures(d):
        assert abs(x - e) <= sagitta, (x, e, sagitta)
    assert d["a_to_b"]["max"] >= d["a_to_b"]["vertex_max"] and d["hausdorff"] == max(d["a_to_b"]["max"], d["b_to_a"]["max"])


# ---- the premises of the GPU cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("sphere", "pair"))
def test_premises_of_the_closest_point_cases(kind):
    v, f, p, r64, r32 = Q.point_case(kind)
    assert bool((r64["face"] >= 0).all())
    compared = r64["runner"] - r64["dist"] > Q.FACE_GAP
    share = float(compared.float().mean())
    print(f"{kind}: face compared on {share:.3f} of the queries; float32 restatement off by {float((r32['dist'].double() - r64['dist']).abs().max()):.3e}")
    # Where the closest point lies on an edge or a vertex, two or more faces are equally near and `face` is compared on none of them: the
    # 100 queries at vertices always, and outside a convex mesh a good part of the others.  A third must remain for (c) to mean something.
    assert share > 1 / 3
    for n in Q.POINT_COUNTS:
        assert bool(compared[:n].any()) or n == 1
    assert int((r64["dist"] == 0).sum()) >= 100             # the queries at vertices
    far = p.abs().min(1).values > 5
    assert int(far.sum()) == 100 and bool((r64["dist"][far] > 4).all())


@pytest.mark.parametrize("case", Q.OCC_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_premises_of_the_occlusion_cases(case):
    name, K, radius = case
    count = max(Q.OCC_COUNTS) if case == Q.OCC_CASES[0] else Q.OCC_SMALL
    o = Q.occ_case(name, K, radius, count)
    assert bool(o["valid"].all())
    rays = count * K
    marginal, sure = int(o["marginal"].sum()), int(o["sure"].sum())
    print(f"{name} K {K} radius {radius}: {sure / rays:.4f} of {rays} rays occluded, {marginal / rays:.5f} marginal, hits {int(o['sure'].min())} .. {int(o['sure'].max())}")
    assert marginal <= Q.MARGINAL_MAX * rays
    assert sure > 0.02 * rays                                # the case does test occlusion
    assert bool((o["sure"] <= o["hits"]).all()) and bool((o["hits"] <= o["sure"] + o["marginal"]).all())


@pytest.mark.parametrize("name", Q.EXTRA_OCC_CASES)
def test_premises_of_the_extra_occlusion_cases(name):
    """The other seed, the points that are not valid and the lifted points with bias 0 of tests/test_mesh_query_gpu.py: the same cap"""
    o, K = Q.extra_occ_case(name)
    valid = o["valid"]
    rays = int(valid.sum()) * K
    marginal = int(o["marginal"][valid].sum())
    print(f"{name}: {marginal} marginal rays of {rays}, {int(o['sure'][valid].sum()) / rays:.4f} occluded")
    assert rays > 0 and marginal <= Q.MARGINAL_MAX * rays and int(o["sure"][valid].sum()) > 0.02 * rays
    if name == "invalid":
        assert (~valid).nonzero().reshape(-1).tolist() == [3, 10, 20, 30, 40] and bool((o["hits"][~valid] == -1).all())


def test_int_arguments_take_numpy_integers():
    assert MQ._int_arg(np.int64(64), 1, 1024, "t", "samples") == 64 and MQ._int_arg(np.uint32(7), 0, 2 ** 32 - 1, "t", "seed") == 7
    assert type(MQ._int_arg(np.int32(3), 1, 16, "t", "subdivide")) is int
    for bad in (2.5, np.float32(2.0), True, np.bool_(True), "3", None, 0, 17):
        with pytest.raises(ValueError, match="subdivide"):
            MQ._int_arg(bad, 1, 16, "t", "subdivide")


@pytest.fixture(scope="module")
def ao_bakes():
    lv, lf, hv, hf, md, radius = Q.ao_scene()
    ln, hn = C.normals(lv, lf).float(), C.normals(hv, hf).float()
    return {R: Q.bake_ao(lv, lf, ln, hv, hf, hn, R, md, 32, radius, Q.AO_BIAS) for R in B.BAKE_SIZES}


@pytest.mark.parametrize("tex", B.BAKE_SIZES)
def test_premises_of_the_ao_bake(ao_bakes, tex):
    b = ao_bakes[tex]
    rows = b["cast"] & b["keep"]
    rays = 32 * int(rows.sum())
    assert int(rows.sum()) > 0.9 * int(b["cast"].sum())
    assert int(b["marginal"][rows].sum()) <= Q.MARGINAL_MAX * rays
    assert bool((b["hits"][~b["cast"]] == -1).all()) and bool((b["hits"][b["cast"]] >= 0).all())
    # dimples are darker than bumps
    ao = 1 - b["hits"][rows].double() / 32
    sign = Q.bump_sign(b["points"][rows])
    dimple, bump = float(ao[sign < -0.3].mean()), float(ao[sign > 0.3].mean())
    print(f"R {tex}: {int(rows.sum())} of {int(b['cast'].sum())} texels kept, {int(b['marginal'][rows].sum())} marginal rays of {rays}; ao over dimples "
          f"{dimple:.4f}, over bumps {bump:.4f}")
    assert dimple < bump - 0.05


# ---- the OBJ writer ---------------------------------------------------------------------------------------------------------------------------
def test_obj_writer_with_and_without_an_ao_map(tmp_path):
    from PIL import Image

    from v3d_amd.recon import mesh_texture as MT
    v, f = M.icosphere(0)
    R = 32
    vt = TX.face_uvs(f.shape[0], R).float()
    g = torch.Generator().manual_seed(0)
    tex, ao = torch.rand(R * R, 3, generator=g), torch.rand(R * R, generator=g) * 1.2 - 0.1
    nm = torch.nn.functional.normalize(torch.randn(R * R, 3, generator=g), dim=1)
    read = lambda p: open(p, "rb").read()  # noqa: E731
    for sub, kw in (("plain", {}), ("nm", {"normal_map": nm})):
        a, b, c = tmp_path / (sub + "_a"), tmp_path / (sub + "_b"), tmp_path / (sub + "_c")
        for d in (a, b, c):
            d.mkdir()
        MT.save_textured_obj(str(a / "m.obj"), v, f, vt, tex, **kw)
        MT.save_textured_obj(str(b / "m.obj"), v, f, vt, tex, ao_map=None, **kw)
        MT.save_textured_obj(str(c / "m.obj"), v, f, vt, tex, ao_map=ao, **kw)
        assert sorted(os.listdir(a)) == sorted(os.listdir(b))
        for name in os.listdir(a):
            assert read(a / name) == read(b / name), name
            if name != "m.mtl":
                assert read(a / name) == read(c / name), name
        assert sorted(os.listdir(c)) == sorted(os.listdir(a) + ["m_ao.png"])
        mtl_a, mtl_c = read(a / "m.mtl").decode(), read(c / "m.mtl").decode()
        assert mtl_c == mtl_a + "map_Ka m_ao.png\n" and "map_Ka" not in mtl_a
        img = Image.open(c / "m_ao.png")
        assert img.mode == "L" and img.size == (R, R)
        assert np.array_equal(np.asarray(img).reshape(-1), np.floor(np.clip(ao.numpy(), 0, 1) * 255.0 + 0.5).astype(np.uint8))
        # the reader ignores the lines it does not know
        rv, rf, rvt, rtex = MT.read_textured_obj(str(c / "m.obj"))
        assert np.array_equal(rf, f.numpy()) and rtex.shape == (R * R, 3)
    with pytest.raises(ValueError, match="occlusion map of 10 texels"):
        MT.save_textured_obj(str(tmp_path / "bad.obj"), v, f, vt, tex, ao_map=torch.zeros(10))


# ---- the scripts and the host API -------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mesh_distance_options_parse():
    mod = _entry("mesh_distance")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh_50k.ply", "--reference", "out/gs/mesh_clean.ply"]))
    assert a == {"mesh": "out/gs/mesh_50k.ply", "reference": "out/gs/mesh_clean.ply", "subdivide": 2, "json": None}
    b = vars(ap.parse_args(["--mesh", "m.obj", "--reference", "r.ply", "--subdivide", "4", "--json", "d.json"]))
    assert (b["subdivide"], b["json"]) == (4, "d.json")
    for bad in (["--mesh", "m.ply"], ["--reference", "r.ply"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    base = ["--mesh", "does/not/exist.ply", "--reference", "does/not/exist.ply"]
    for bad in (["--subdivide", "0"], ["--subdivide", "17"], ["--json", "out.txt"]):
        with pytest.raises(SystemExit):                    # refused before anything is read
            mod.main(base + bad)
    for bad in (["--mesh", "does/not/exist.glb", "--reference", "does/not/exist.ply"], ["--mesh", "does/not/exist.ply", "--reference", "does/not/exist.obj"]):
        with pytest.raises(SystemExit):
            mod.main(bad)


def test_bake_ao_options_parse():
    mod = _entry("bake_ao")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh_50k_nm.obj", "--high", "out/gs/mesh_clean.ply", "-o", "out/gs/ao.obj"]))
    assert a == {"mesh": "out/gs/mesh_50k_nm.obj", "high": "out/gs/mesh_clean.ply", "out": "out/gs/ao.obj", "white_background": False,
                 "texture_resolution": 1024, "samples": 64, "ao_radius": None, "ao_bias": None, "max_dist": None, "reso": 512, "radius": 2.0,
                 "elevation": 0.0, "fov": 60.0, "render_orbit": 0}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov"):
        assert a[k] == recon[k], k
    b = vars(ap.parse_args(["--mesh", "m.ply", "--high", "h.ply", "--samples", "16", "--ao_radius", "0.2", "--ao_bias", "0", "--max_dist", "0.01",
                            "--texture_resolution", "2048", "--render_orbit", "36", "-w"]))
    assert (b["samples"], b["ao_radius"], b["ao_bias"], b["max_dist"], b["texture_resolution"], b["render_orbit"], b["white_background"], b["out"]) == \
        (16, 0.2, 0.0, 0.01, 2048, 36, True, None)
    for bad in (["--high", "h.ply"], ["--mesh", "m.ply"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    base = ["--mesh", "does/not/exist.ply", "--high", "does/not/exist.ply"]
    for bad in (["--texture_resolution", "0"], ["--texture_resolution", "4097"], ["--samples", "0"], ["--samples", "1025"], ["--ao_radius", "0"],
                ["--ao_radius", "inf"], ["--ao_radius", "nan"], ["--ao_bias", "-1"], ["--ao_bias", "nan"], ["--max_dist", "-1"], ["--max_dist", "inf"],
                ["-o", "out.ply"], ["--render_orbit", "-1"], ["--reso", "0"]):
        with pytest.raises(SystemExit):                    # refused before anything is read
            mod.main(base + bad)
    with pytest.raises(SystemExit):
        mod.main(["--mesh", "does/not/exist.glb", "--high", "does/not/exist.ply"])


def test_bake_ao_keeps_the_normal_map_of_its_input(tmp_path):
    from v3d_amd.recon import mesh_texture as MT
    mod = _entry("bake_ao")
    v, f = M.icosphere(0)
    R = 32
    vt = TX.face_uvs(f.shape[0], R).float()
    g = torch.Generator().manual_seed(0)
    tex, nm = torch.rand(R * R, 3, generator=g), torch.nn.functional.normalize(torch.randn(R * R, 3, generator=g), dim=1)
    MT.save_textured_obj(str(tmp_path / "in.obj"), v, f, vt, tex, normal_map=nm)
    MT.save_textured_obj(str(tmp_path / "plain.obj"), v, f, vt, tex)
    assert mod.normal_map_of(str(tmp_path / "plain.obj")) is None
    png = mod.normal_map_of(str(tmp_path / "in.obj"))
    assert png == str(tmp_path / "in_normal.png")
    MT.save_textured_obj(str(tmp_path / "out.obj"), v, f, vt, tex, ao_map=torch.rand(R * R, generator=g))
    mod.keep_normal_map(png, str(tmp_path / "out"))
    assert open(tmp_path / "out_normal.png", "rb").read() == open(png, "rb").read()
    lines = open(tmp_path / "out.mtl").read().splitlines()
    assert lines[-3:] == ["map_Kd out.png", "norm out_normal.png", "map_Ka out_ao.png"]
    assert mod.normal_map_of(str(tmp_path / "out.obj")) == str(tmp_path / "out_normal.png")
    # file names with spaces
    MT.save_textured_obj(str(tmp_path / "two words.obj"), v, f, vt, tex, normal_map=nm)
    assert mod.normal_map_of(str(tmp_path / "two words.obj")) == str(tmp_path / "two words_normal.png")
    # a normal map that the MTL names and that is not there: refused before anything is baked or written
    os.remove(tmp_path / "in_normal.png")
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit, match="in_normal.png"):
        mod.main(["--mesh", str(tmp_path / "in.obj"), "--high", str(tmp_path / "does_not_exist.ply"), "-o", str(tmp_path / "never.obj")])
    assert sorted(os.listdir(tmp_path)) == before


def test_host_api_refuses_bad_arguments_and_answers_the_empty_cases_without_a_launch():
    v, f = M.icosphere(0)
    none_f, none_v = torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3)
    for args in ((v, none_f, v, f), (v, f, v, none_f), (none_v, none_f, v, f)):
        with pytest.raises(ValueError, match="nothing to measure"):
            MQ.mesh_distance(*args, device="cpu")
    with pytest.raises(ValueError, match="subdivide 0"):
        MQ.mesh_distance(v, f, v, f, subdivide=0, device="cpu")
    with pytest.raises(ValueError, match="subdivide 17"):
        MQ.face_samples(v, f, subdivide=17, device="cpu")
    with pytest.raises(ValueError):
        MQ.mesh_distance(v, torch.tensor([[0, 1, 99]]), v, f, device="cpu")                      # a face outside the vertex array
    pts, w = MQ.face_samples(v, none_f, device="cpu")
    assert tuple(pts.shape) == (0, 3) and tuple(w.shape) == (0,)
    # a tree that is never walked: the refusals and the empty cases come first
    from v3d_amd.recon.mesh_bake import MeshBVH
    z = torch.zeros(1, dtype=torch.int32)
    bvh = MeshBVH(v, f.int(), z, z, z, z, torch.zeros(1, 3), torch.zeros(1, 3), 0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            MQ.closest_points(bvh, torch.zeros(4, 3), max_dist=bad)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        MQ.closest_points(bvh, torch.zeros(4, 2))
    d, face, uv = MQ.closest_points(bvh, torch.zeros(0, 3))
    assert tuple(d.shape) == (0,) and face.dtype == torch.int32 and tuple(uv.shape) == (0, 2)
    for kw, what in ((dict(samples=0), "samples 0"), (dict(samples=1025), "samples 1025"), (dict(samples=2.5), "samples"), (dict(radius=0.0), "radius"),
                     (dict(radius=INF), "radius"), (dict(bias=-1e-3), "bias"), (dict(bias=float("nan")), "bias"), (dict(seed=-1), "seed"),
                     (dict(seed=2 ** 32), "seed")):
        with pytest.raises(ValueError, match=what):
            MQ.occlusion(bvh, torch.zeros(4, 3), torch.ones(4, 3), **kw)
    with pytest.raises(ValueError, match="4 points, 3 normals"):
        MQ.occlusion(bvh, torch.zeros(4, 3), torch.ones(3, 3))
    hits = MQ.occlusion(bvh, torch.zeros(0, 3), torch.zeros(0, 3))
    assert tuple(hits.shape) == (0,) and hits.dtype == torch.int32
    # the bake
    for kw, what in ((dict(tex_size=0), "tex_size 0"), (dict(samples=0), "samples 0"), (dict(radius=-1.0), "radius"), (dict(bias=INF), "bias"),
                     (dict(max_dist=INF), "max_dist")):
        with pytest.raises(ValueError, match=what):
            MQ.bake_ambient_occlusion(v, f, v, f, device="cpu", **{"tex_size": 64, **kw})
    with pytest.raises(ValueError, match="no faces to hit"):
        MQ.bake_ambient_occlusion(v, f, v, none_f, tex_size=64, device="cpu")
    for vv, ff in ((v, none_f), (none_v, none_f)):
        ao, stats = MQ.bake_ambient_occlusion(vv, ff, v, f, tex_size=16, samples=8, device="cpu")
        assert tuple(ao.shape) == (256,) and bool((ao == 1).all()) and stats["owned"] == 0 and stats["rays"] == 0 and stats["samples"] == 8
    ao, _ = MQ.bake_ambient_occlusion(none_v, none_f, none_v, none_f, tex_size=8, device="cpu")
    assert bool((ao == 1).all())
