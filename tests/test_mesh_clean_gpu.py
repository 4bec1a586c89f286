"""The gfx950 mesh cleaning (csrc_recon/meshtopo.hip, v3d_amd/recon/mesh_clean.py, scripts/pub/clean_mesh.py) against the torch restatement
(tests/mesh_clean_ref.py): the vertex -> corner lists, normals, connected components, the component filter, boundary flags, Taubin
smoothing, the normal render, the entry point, and the empty cases.

Integer outputs (ranges, corner lists, labels, round counts, component tables, kept faces, remapped indices, boundary flags) are exact.
Float outputs follow the rule of tests/test_mesh_render_gpu.py and tests/test_mesh_refine_gpu.py: the kernel may be off from the fp64
restatement by 4x what the restatement's own float32 run is off, or by 2^-23 x the largest magnitude in the array when that is larger
(mesh_clean_ref.float_bar).  Both figures of every scene go to the parity record."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_clean_ref as C
import mesh_render_ref as M
import recon_geom_ref as R
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_clean as MC
from v3d_amd.recon import mesh_render as MR
from v3d_amd.recon.cameras import orbit_cameras

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z_UP = torch.tensor([0.0, 0.0, 1.0])


@functools.lru_cache(maxsize=None)
def scene(name):
    """(verts, faces, colors) on the host, built once and shared (nothing below writes into them)"""
    if name in ("sphere", "pair"):
        return M.mesh_scene(name, M.SEEDS[name])
    if name == "unreferenced":
        return C.insert_unreferenced(*scene("sphere"))[:3]
    if name == "degenerate":
        return C.add_degenerate(*scene("unreferenced"))
    return {"fan": C.fan, "triangle": C.triangle, "floaters": lambda: C.floater_scene()[:3], "strip": lambda: C.quad_strip(500, seed=4)[:3],
            "net": C.sphere_mesh, "noisy": lambda: C.noisy_sphere(0), "grid": C.open_grid}[name]()


@functools.lru_cache(maxsize=None)
def extracted_sphere():
    """The 24^3 sphere through the project's own surface nets, on the device"""
    N = C.SPHERE["N"]
    ref = R.sphere_volume(N, C.SPHERE["bound"], C.SPHERE["radius"])
    f32 = lambda t, *s: t.float().reshape(*s).contiguous().to(DEV)  # noqa: E731
    vol = G.TsdfVolume(N, ref["bound"], ref["trunc"], f32(ref["tsdf_sum"], N, N, N), f32(ref["weight"], N, N, N), f32(ref["rgb_sum"], 3, N, N, N),
                       f32(ref["rgb_weight"], N, N, N))
    return G.extract_mesh(vol)


# ---- 1. adjacency -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sphere", "pair", "fan", "triangle", "unreferenced"))
def test_corner_lists_match_the_restatement(name):
    v, f, _ = scene(name)
    V = v.shape[0]
    ranges, corners = MC.vertex_corners(f, V)
    want_ranges, want_corners = C.corner_lists(f, V)
    assert ranges.dtype == torch.int32 and corners.dtype == torch.int32 and tuple(ranges.shape) == (V, 2) and corners.numel() == 3 * f.shape[0]
    assert torch.equal(ranges.cpu().long(), want_ranges) and torch.equal(corners.cpu().long(), want_corners)
    length = want_ranges[:, 1] - want_ranges[:, 0]
    if name == "fan":
        assert int(length[0]) == C.FAN > 256                           # one list is longer than any block
    if name == "unreferenced":
        assert int((length == 0).sum()) == 5 and bool((want_ranges[length == 0] == 0).all())
    again = MC.vertex_corners(f, V)
    assert torch.equal(again[0], ranges) and torch.equal(again[1], corners)


# ---- 2. normals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sphere", "pair", "fan", "triangle", "unreferenced", "degenerate", "net"))
def test_normals_match_the_restatement(name):
    v, f, _ = scene(name)
    out = MC.vertex_normals(v, f).cpu()
    n64, n32 = C.normals(v, f), C.normals(v, f, torch.float32)
    err, err32, bound = C.float_bar(out, n64, n32)
    none = ~C.has_normal(v, f)
    print(f"{name}: normals {err:.3e} from fp64 (float32 restatement {err32:.3e}, bound {bound:.3e}); {int(none.sum())} default normals")
    record_parity(f"mesh_clean_normals[{name}]", {"max_abs": err, "float32_restatement": err32, "bound": bound, "default_normals": int(none.sum())})
    assert torch.equal(out[none], Z_UP.expand(int(none.sum()), 3))
    assert int(none.sum()) == {"unreferenced": 5, "degenerate": 11}.get(name, 0)
    assert float((out.norm(dim=1) - 1).abs().max()) < 1e-6
    assert err <= bound
    assert torch.equal(MC.vertex_normals(v, f).cpu(), out)


# ---- 3. components ------------------------------------------------------------------------------------------------------------------------
def test_components_of_the_floater_scene():
    v, f, _ = scene("floaters")
    V = v.shape[0]
    labels, rounds = MC.vertex_components(f, V)
    want, want_rounds = C.components(f, V)
    assert labels.dtype == torch.int32 and torch.equal(labels.cpu().long(), want) and rounds == want_rounds
    assert len(set(want.tolist())) == 5 + 3                           # two spheres, two triangles, a tetrahedron; three loose vertices
    again, rounds2 = MC.vertex_components(f, V)
    assert torch.equal(again, labels) and rounds2 == rounds
    record_parity("mesh_clean_components[floaters]", {"vertices": V, "rounds": rounds, "rounds_restatement": want_rounds})


def test_components_of_a_permuted_strip_take_hundreds_of_rounds():
    v, f, _ = scene("strip")
    V = v.shape[0]
    labels, rounds = MC.vertex_components(f, V)
    want, want_rounds = C.components(f, V)
    _, slow_rounds = C.components(f, V, jump=False)
    print(f"strip of 500 quads, permuted: {rounds} rounds (restatement {want_rounds}, without the jump {slow_rounds})")
    record_parity("mesh_clean_components[strip]", {"vertices": V, "rounds": rounds, "rounds_restatement": want_rounds, "rounds_without_jump": slow_rounds})
    assert not labels.any() and torch.equal(labels.cpu().long(), want)                 # one component: its smallest index is 0
    assert rounds == want_rounds and 100 < rounds <= V + 8 and rounds > 3 * MC.ROUND_GROUP     # several reads of the flags


def test_extracted_sphere_is_one_component():
    verts, faces, _ = extracted_sphere()
    labels, rounds = MC.vertex_components(faces, verts.shape[0])
    want, want_rounds = C.components(faces.cpu().long(), verts.shape[0])
    record_parity("mesh_clean_components[net]", {"vertices": verts.shape[0], "rounds": rounds, "rounds_restatement": want_rounds})
    assert not labels.any() and rounds == want_rounds == 6


def test_faces_with_an_index_out_of_range_are_absent():
    """Below the host's validation: three faces with an index of -1, V and INT32_MAX behind the sphere's own leave every result as it was"""
    v, f, _ = scene("sphere")
    V, F = v.shape[0], f.shape[0]
    bad = torch.cat([f, torch.tensor([[-1, 0, 1], [0, V, 1], [2, 3, 2 ** 31 - 1]])]).to(DEV, torch.int32).contiguous()
    good = f.to(DEV, torch.int32).contiguous()
    vd = v.to(DEV)
    lists, blists = MC._corner_lists(good, V), MC._corner_lists(bad, V)
    assert torch.equal(MC._normals(vd, bad, *blists), MC._normals(vd, good, *lists))
    (labels, rounds), (blabels, brounds) = MC._labels(good, V, *lists), MC._labels(bad, V, *blists)
    assert torch.equal(blabels, labels) and brounds == rounds
    assert MC._component_table(bad, V, blabels) == MC._component_table(good, V, labels) == [{"root": 0, "faces": F, "vertices": V}]
    assert torch.equal(MC._boundary(bad, V, *blists), MC._boundary(good, V, *lists)) and not MC._boundary(bad, V, *blists).any()
    assert torch.equal(MC._smooth(vd, bad, *blists, None, 2, 0.5, -0.53), MC._smooth(vd, good, *lists, None, 2, 0.5, -0.53))
    bv, bf, _, _ = MC._compact(vd, bad, None, *blists, blabels, [0])
    assert torch.equal(bv, vd) and torch.equal(bf, good)


# ---- 4. filter ----------------------------------------------------------------------------------------------------------------------------
def test_filter_drops_floaters_and_keeps_the_order():
    v, f, c = scene("floaters")
    V, F = v.shape[0], f.shape[0]
    fv, ff, fc, stats = MC.filter_components(v, f, c, min_faces=8)
    wv, wf, wc, keep_face, keep_vert, table = C.filter_components(v, f, c, min_faces=8)
    assert fv.shape[0] == 324 and ff.shape[0] == 640 and ff.dtype == torch.int32
    assert torch.equal(fv.cpu(), wv) and torch.equal(fc.cpu(), wc) and torch.equal(ff.cpu().long(), wf)
    assert torch.equal(fv.cpu()[ff.cpu().long()], v[f[keep_face]])                     # the same triangles in the same order
    assert stats["components_before"] == table and [r["faces"] for r in stats["components_after"]] == [320, 320]
    labels_after, _ = C.components(wf, 324)
    assert [r["root"] for r in stats["components_after"]] == sorted(set(labels_after.tolist()))
    assert stats["removed_faces"] == F - 640 == 6 and stats["removed_vertices"] == V - 324 == 13 and stats["unreferenced_vertices"] == 3
    json.loads(json.dumps(stats, allow_nan=False))
    # keep_largest = 1 with two components of 320 faces: the one with the smaller root
    kv, kf, kc, kstats = MC.filter_components(v, f, c, min_faces=0, keep_largest=1)
    big = sorted(r["root"] for r in table if r["faces"] == 320)
    labels, _ = C.components(f, V)
    assert kf.shape[0] == 320 and kv.shape[0] == 162 and torch.equal(kv.cpu(), v[labels == big[0]])
    wv1, wf1, _, _, _, _ = C.filter_components(v, f, c, min_faces=0, keep_largest=1)
    assert torch.equal(kv.cpu(), wv1) and torch.equal(kf.cpu().long(), wf1)
    # both rules, and min_faces alone at the size of the spheres
    bv, bf, _, _ = MC.filter_components(v, f, c, min_faces=320, keep_largest=5)
    assert torch.equal(bv, fv) and torch.equal(bf, ff)
    # nothing to remove: bit-equal
    sv, sf, sc = scene("net")
    ov, of, oc, ostats = MC.filter_components(sv, sf, sc)
    assert torch.equal(ov.cpu(), sv) and torch.equal(oc.cpu(), sc) and torch.equal(of.cpu().long(), sf)
    assert ostats["removed_faces"] == 0 == ostats["removed_vertices"] and ostats["components_after"] == ostats["components_before"]
    # everything below min_faces: nothing is left
    ev, ef, ec, estats = MC.filter_components(v, f, c, min_faces=321)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ec.shape == (0, 3) and estats["removed_faces"] == F and estats["components_after"] == []


# ---- 5. boundary --------------------------------------------------------------------------------------------------------------------------
def test_boundary_flags():
    v, f, _ = scene("grid")
    flags = MC.boundary_vertices(f, v.shape[0])
    want = C.boundary_flags(f, v.shape[0])
    assert flags.dtype == torch.int32 and torch.equal(flags.cpu().long(), want) and 0 < int(want.sum()) < v.shape[0]
    for name in ("sphere", "net", "pair"):
        vv, ff, _ = scene(name)
        assert not MC.boundary_vertices(ff, vv.shape[0]).any(), name
    vv, ff, _ = scene("fan")                                           # a list of 700 entries: the ring is open, the centre is not
    assert MC.boundary_vertices(ff, vv.shape[0]).cpu().tolist() == [0] + [1] * C.FAN
    vv, ff, _ = scene("floaters")
    assert torch.equal(MC.boundary_vertices(ff, vv.shape[0]).cpu().long(), C.boundary_flags(ff, vv.shape[0]))


# ---- 6. smoothing -------------------------------------------------------------------------------------------------------------------------
def test_taubin_smoothing_matches_the_restatement():
    v, f, _ = scene("noisy")
    out = MC.taubin_smooth(v, f, iterations=10, lam=0.5, mu=-0.53)
    p64, p32 = C.taubin(v, f), C.taubin(v, f, dtype=torch.float32)
    err, err32, bound = C.float_bar(out.cpu(), p64, p32)
    vol0 = R.signed_volume(v, f)
    ratio, want_ratio = R.signed_volume(out.cpu(), f) / vol0, R.signed_volume(p64, f) / vol0
    rough = float(out.cpu().double().norm(dim=1).std()) / float(v.double().norm(dim=1).std())
    print(f"noisy sphere, 10 iterations: positions {err:.3e} from fp64 (float32 restatement {err32:.3e}, bound {bound:.3e}); volume ratio {ratio:.6f} "
          f"(restatement {want_ratio:.6f}); std |v| ratio {rough:.3f}")
    record_parity("mesh_clean_taubin[noisy0]", {"max_abs": err, "float32_restatement": err32, "bound": bound, "volume_ratio": ratio,
                                                "volume_ratio_restatement": want_ratio, "roughness_ratio": rough})
    assert err <= bound
    assert abs(ratio - want_ratio) <= 1e-5
    assert torch.equal(MC.taubin_smooth(v, f), out)                    # the defaults; two runs are bit-equal
    # still closed: no pixel of any camera sees an odd number of faces
    for cam in D.cams_for(64, 64, n=4, elevation=15.0):
        hits = MR.render_mesh(cam, out, f, torch.zeros_like(out), [1.0, 1.0, 1.0], cull=False, count_hits=True)["n_hit"]
        assert int(hits.max()) >= 2 and int((hits % 2 == 1).sum()) == 0


def test_fix_boundary_pins_the_open_edges():
    v, f, _ = scene("grid")
    flags = C.boundary_flags(f, v.shape[0]).bool()
    out = MC.taubin_smooth(v, f, iterations=3, fix_boundary=True).cpu()
    assert torch.equal(out[flags], v[flags]) and bool((out[~flags] != v[~flags]).any(1).all())
    p64, p32 = C.taubin(v, f, 3, fix_boundary=True), C.taubin(v, f, 3, fix_boundary=True, dtype=torch.float32)
    err, err32, bound = C.float_bar(out, p64, p32)
    free = MC.taubin_smooth(v, f, iterations=3).cpu()
    ferr, ferr32, fbound = C.float_bar(free, C.taubin(v, f, 3), C.taubin(v, f, 3, dtype=torch.float32))
    record_parity("mesh_clean_taubin[grid]", {"pinned_max_abs": err, "pinned_float32_restatement": err32, "pinned_bound": bound, "free_max_abs": ferr,
                                              "free_float32_restatement": ferr32, "free_bound": fbound})
    assert err <= bound and ferr <= fbound and bool((free[flags] != v[flags]).any())


# ---- 7. normal render ---------------------------------------------------------------------------------------------------------------------
def test_normal_render_of_a_sphere():
    """An icosphere of 1280 faces at the origin from an orbit camera at elevation 0, whose axis goes through the sphere's centre.  The image
    centre lies between the four middle pixels of 64 x 64: pixel (32, 32) looks half a pixel right of and below it, at a point of the sphere
    0.5 * 1.5 / 55.4 = 0.0135 off the axis, whose normal is tilted by 0.0135 / 0.5 = 0.027: 0.0135 in colour, inside the 0.02."""
    S = 64
    v, f = M.icosphere(3, 0.5)
    cam = orbit_cameras(1, 2.0, 0.0, 60.0, S)[0][0]
    bg = (0.25, 0.5, 0.75)
    towards = (cam.center / cam.center.norm()).expand(v.shape[0], 3)
    flat = MC.render_mesh_normals(cam, v, f, normals=towards, bg=bg)
    hit = flat["alpha"].cpu() > 0
    assert 0.1 < float(hit.float().mean()) < 0.5
    img = flat["render"].cpu()
    assert float((img[:, hit] - torch.tensor([0.5, 0.5, 1.0])[:, None]).abs().max()) < 1e-5      # a normal that points at the camera
    assert torch.equal(img[:, ~hit], torch.tensor(bg)[:, None].expand(3, int((~hit).sum())))
    out = MC.render_mesh_normals(cam, v, f, bg=bg)
    img = out["render"].cpu()
    assert torch.equal(out["alpha"].cpu() > 0, hit) and torch.equal(img[:, ~hit], torch.tensor(bg)[:, None].expand(3, int((~hit).sum())))
    mid, step = S // 2, 8
    centre = img[:, mid, mid]
    print(f"centre pixel {centre.tolist()}")
    record_parity("mesh_clean_normal_render", {"centre_pixel": centre.tolist()})
    assert float((centre - torch.tensor([0.5, 0.5, 1.0])).abs().max()) < 0.02
    assert hit[mid, mid - step] and hit[mid, mid + step] and hit[mid - step, mid] and hit[mid + step, mid]
    assert float(img[0, mid, mid - step]) < float(centre[0]) < float(img[0, mid, mid + step])     # red rises to the right
    assert float(img[1, mid + step, mid]) < float(centre[1]) < float(img[1, mid - step, mid])     # green rises upwards (rows run down)
    frames = MC.render_normal_orbit(v, f, 2, 2.0, 0.0, 60.0, S, True)
    assert frames.shape == (2, S, S, 3) and frames.dtype == np.uint8
    assert np.array_equal(frames[0], (MC.render_mesh_normals(cam, v, f)["render"].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy())


# ---- 8. the whole, and the entry point ------------------------------------------------------------------------------------------------------
def planted():
    """The extracted sphere with a floating triangle, a floating tetrahedron and a loose vertex behind it"""
    verts, faces, colors = extracted_sphere()
    V = verts.shape[0]
    extra = torch.tensor([[0.8, 0.8, 0.8], [0.85, 0.8, 0.8], [0.8, 0.85, 0.82], [0.7, -0.7, 0.0], [0.75, -0.7, 0.0], [0.7, -0.65, 0.0], [0.72, -0.68, 0.05],
                          [0.0, 0.0, 0.9]], device=DEV)
    ef = torch.tensor([[0, 1, 2], [3, 5, 4], [3, 4, 6], [4, 5, 6], [5, 3, 6]], dtype=torch.int32, device=DEV) + V
    return torch.cat([verts, extra]), torch.cat([faces, ef]), torch.cat([colors, torch.full((8, 3), 0.5, device=DEV)])


def test_clean_mesh_filters_then_smooths():
    verts, faces, colors = extracted_sphere()
    pv, pf, pc = planted()
    ov, of, oc, stats = MC.clean_mesh(pv, pf, pc, min_faces=64, iterations=4)
    assert torch.equal(of, faces) and torch.equal(oc, colors)
    assert torch.equal(ov, MC.taubin_smooth(verts, faces, iterations=4))
    assert stats["faces_before"] == faces.shape[0] + 5 and stats["faces"] == faces.shape[0] and stats["vertices"] == verts.shape[0]
    assert stats["removed_faces"] == 5 and stats["removed_vertices"] == 8 and stats["unreferenced_vertices"] == 1 and stats["rounds"] == 6
    assert [r["faces"] for r in stats["components_before"]] == [faces.shape[0], 1, 4] and stats["components_after"] == stats["components_before"][:1]
    assert stats["boundary_vertices_before"] == 3 and stats["boundary_vertices_after"] == 0       # the floating triangle is all rim
    json.loads(json.dumps(stats, allow_nan=False))
    nv, nf, nc, nstats = MC.clean_mesh(pv, pf, pc, min_faces=0, iterations=0)         # both steps off: the mesh as it came
    assert torch.equal(nv, pv) and torch.equal(nf, pf) and torch.equal(nc, pc) and not nstats["filtered"] and nstats["removed_vertices"] == 0
    assert nstats["components_after"] == nstats["components_before"] == stats["components_before"] and nstats["unreferenced_vertices"] == 1


def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_clean_mesh_script_end_to_end(tmp_path):
    verts, faces, colors = extracted_sphere()
    pv, pf, pc = planted()
    ply, out = str(tmp_path / "mesh.ply"), str(tmp_path / "mesh_clean.ply")
    G.save_mesh_ply(ply, pv, pf, pc)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pub", "clean_mesh.py"), "--mesh", ply, "-o", out, "--min_faces", "64", "--smooth", "3",
                        "--render_normals", "2", "--reso", "64", "-w"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "components 3 -> 1" in r.stdout and "removed 5 triangles and 8 vertices" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["mesh.ply", "mesh_clean.json", "mesh_clean.ply", "mesh_clean_normals"]
    assert sorted(os.listdir(tmp_path / "mesh_clean_normals")) == ["000.png", "001.png", "orbit.npy"]
    stats = json.load(open(tmp_path / "mesh_clean.json"))
    assert stats["faces"] == faces.shape[0] and stats["vertices"] == verts.shape[0] and stats["removed_faces"] == 5 and stats["removed_vertices"] == 8
    assert stats["unreferenced_vertices"] == 1 and stats["smooth_iterations"] == 3 and stats["boundary_vertices_after"] == 0 and stats["rounds"] == 6
    rv, rf, rc = G.read_mesh_ply(out)
    assert np.array_equal(rf, faces.cpu().numpy()) and rv.shape == (verts.shape[0], 3)
    assert np.array_equal(rv, MC.taubin_smooth(verts, faces, iterations=3).cpu().numpy())
    assert np.array_equal(rc, np.rint(np.clip(colors.cpu().numpy(), 0, 1) * 255).astype(np.uint8))             # the colours ride along
    frames = np.load(tmp_path / "mesh_clean_normals" / "orbit.npy")
    assert frames.shape == (2, 64, 64, 3) and frames.dtype == np.uint8 and bool((frames[:, 0, 0] == 255).all()) and bool((frames != 255).any())
    # render_mesh.py takes the output unchanged (in this process: the script under test above ran in its own)
    orbit = str(tmp_path / "orbit")
    _entry("render_mesh").main(["--mesh", out, "-o", orbit, "--render_orbit", "1", "--reso", "32", "-w"])
    assert sorted(os.listdir(orbit)) == ["000.png", "orbit.npy"]


# ---- 9. empty cases -----------------------------------------------------------------------------------------------------------------------
def test_empty_meshes_on_the_device():
    v, f, c = scene("floaters")
    none = torch.zeros(0, 3, dtype=torch.int64)
    for vv, cc in ((v, c), (v[:0], c[:0])):
        V = vv.shape[0]
        ranges, corners = MC.vertex_corners(none, V)
        assert ranges.device.type == "cuda" and tuple(ranges.shape) == (V, 2) and not ranges.any() and corners.numel() == 0
        assert MC.vertex_components(none, V)[0].cpu().tolist() == list(range(V))
        assert torch.equal(MC.vertex_normals(vv, none).cpu(), Z_UP.expand(V, 3)) and not MC.boundary_vertices(none, V).any()
        assert torch.equal(MC.taubin_smooth(vv, none).cpu(), vv)
        ov, of, oc, stats = MC.clean_mesh(vv, none, cc)
        assert ov.shape == (0, 3) and of.shape == (0, 3) and oc.shape == (0, 3) and stats["removed_vertices"] == V
    ov, of, oc, stats = MC.clean_mesh(v, f, c, min_faces=1000)         # faces present, every component below min_faces
    assert ov.shape == (0, 3) and of.shape == (0, 3) and oc.shape == (0, 3) and of.dtype == torch.int32
    assert stats["faces"] == 0 == stats["vertices"] and stats["removed_faces"] == f.shape[0] and stats["components_after"] == []
    assert stats["boundary_vertices_before"] == 6 and stats["boundary_vertices_after"] == 0
    out = MC.render_mesh_normals(D.cams_for(40, 24)[0], ov, of)
    assert bool((out["render"] == 1).all()) and not out["alpha"].any()
