"""The gfx950 mesh decimation (csrc_recon/meshdecim.hip, v3d_amd/recon/mesh_decimate.py, scripts/pub/decimate_mesh.py) against the
restatement (tests/mesh_decimate_ref.py): quadrics and costs, which collapses are valid, the selection, the last round's cut, the apply
step, whole runs, the entry point chained into the other mesh scripts, and the cases with nothing to do.

Decisions (who proposes, who is accepted, which faces die, indices) are exact.  Floats follow the rule of tests/test_mesh_clean_gpu.py: the
kernel may be off from the fp64 restatement by 4x what the restatement's own float32 run is off, or by 2^-23 x the largest magnitude in the
array when that is larger (mesh_clean_ref.float_bar).  A flip decision is compared only where the restatement's n_before . n_after lies
further from 0 than its float32 run is off.  The figures go to the parity record."""
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
import mesh_decimate_ref as Dm
import recon_geom_ref as R
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_decimate as MD
from v3d_amd.recon import mesh_render as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_KEY = Dm.NO_KEY


def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def scene(name):
    """(verts, faces, colors) on the host, built once; "extracted" is the 24^3 sphere through the project's own surface nets"""
    if name != "extracted":
        return Dm.scene(name)
    N = C.SPHERE["N"]
    ref = R.sphere_volume(N, C.SPHERE["bound"], C.SPHERE["radius"])
    f32 = lambda t, *s: t.float().reshape(*s).contiguous().to(DEV)  # noqa: E731
    vol = G.TsdfVolume(N, ref["bound"], ref["trunc"], f32(ref["tsdf_sum"], N, N, N), f32(ref["weight"], N, N, N), f32(ref["rgb_sum"], 3, N, N, N),
                       f32(ref["rgb_weight"], N, N, N))
    v, f, c = G.extract_mesh(vol)
    return v.cpu(), f.cpu().long(), c.cpu()


@functools.lru_cache(maxsize=None)
def restated(name, cap=Dm.DEFAULT_MAX_VALENCE):
    """The restatement of one round's first half on a scene, computed once: faces, Q and the analysis in both precisions, keys and targets"""
    v, f, _ = scene(name)
    faces = Dm.face_list(f)
    Q64, Q32 = Dm.vertex_quadrics(v, faces), Dm.vertex_quadrics(v, faces, np.float32)
    i64, i32 = Dm.analyse(v, faces, Q64, cap), Dm.analyse(v, faces, Q32, cap, np.float32)
    keys, targets = Dm.propose(v, faces, Q64, cap, info=i64)
    return dict(faces=faces, Q64=Q64, Q32=Q32, i64=i64, i32=i32, keys=keys, targets=targets)


@functools.lru_cache(maxsize=None)
def kernel_round(name, cap=Dm.DEFAULT_MAX_VALENCE):
    """(Q, keys, targets) of the kernels on a scene, on the host; keys as python ints below 2^64"""
    v, f, _ = scene(name)
    Q = MD.vertex_quadrics(v, f)
    keys, targets = MD.propose(v, f, Q, max_valence=cap)
    return Q.cpu(), keys.cpu(), [k & NO_KEY for k in keys.tolist()], targets.cpu().tolist()


def clear_of_the_flip_threshold(ref):
    return Dm.clear_of_the_flip_threshold(ref["i64"], ref["i32"])


def bar(err, err32, magnitude):
    return max(4.0 * err32, 2.0 ** -23 * magnitude)


# ---- 1. quadrics and costs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ico2", "ico3", "extracted", "noisy"))
def test_quadrics_and_costs_match_the_restatement(name):
    v, f, _ = scene(name)
    ref = restated(name)
    Q, _, keys, targets = kernel_round(name)
    assert Q.dtype == torch.float64 and tuple(Q.shape) == (v.shape[0], 10)
    err, err32, bound = C.float_bar(Q, torch.from_numpy(ref["Q64"]), torch.from_numpy(ref["Q32"]))
    clear = clear_of_the_flip_threshold(ref)
    # the proposed cost against the restatement's cost of the same collapse, and the chosen collapse against the restatement's cheapest
    got, want, want32, best = [], [], [], []
    for vtx, (key, u) in enumerate(zip(keys, targets)):
        cand = ref["i64"][vtx]
        valid = {} if cand is None else {w: c for w, c in cand.items() if not c["why"]}
        if clear[vtx]:
            assert (key != NO_KEY) == bool(valid) and (u >= 0) == bool(valid), vtx               # who proposes: exact
        if key == NO_KEY or not clear[vtx]:
            continue
        assert key & 0xFFFFFFFF == vtx and u in valid, vtx
        got.append(Dm.bits_cost(key >> 32))
        want.append(max(0.0, valid[u]["cost"]))
        want32.append(max(0.0, float(ref["i32"][vtx][u]["cost"])))
        best.append(max(0.0, min(c["cost"] for c in valid.values())))
    got, want, want32, best = (np.asarray(x, dtype=np.float64) for x in (got, want, want32, best))
    cerr, cerr32 = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
    cbound = bar(cerr, cerr32, float(want.max()))
    excess = float((want - best).max())
    same = sum(int(k == r) for k, r in zip(keys, ref["keys"]))
    print(f"{name}: quadrics {err:.3e} from fp64 (float32 restatement {err32:.3e}, bound {bound:.3e}); costs {cerr:.3e} ({cerr32:.3e}, bound {cbound:.3e}); "
          f"chosen above cheapest by {excess:.3e}; {len(got)} proposals, {same} of {len(keys)} keys bit-equal, {clear.count(False)} vertices near a flip")
    record_parity(f"mesh_decimate_quadrics[{name}]", {"max_abs": err, "float32_restatement": err32, "bound": bound, "cost_max_abs": cerr,
                                                      "cost_float32_restatement": cerr32, "cost_bound": cbound, "chosen_above_cheapest": excess,
                                                      "proposals": len(got), "keys_bit_equal": same, "vertices": len(keys)})
    assert err <= bound and cerr <= cbound and excess <= cbound
    assert len(got) >= 0.9 * v.shape[0]
    again = MD.propose(v, f, MD.vertex_quadrics(v, f))
    assert [k & NO_KEY for k in again[0].tolist()] == keys and again[1].tolist() == targets


# ---- 2. validity --------------------------------------------------------------------------------------------------------------------------
def assert_proposals_are_the_restatements(name, cap=Dm.DEFAULT_MAX_VALENCE):
    ref = restated(name, cap)
    _, _, keys, targets = kernel_round(name, cap)
    clear = clear_of_the_flip_threshold(ref)
    assert all(clear), name                                             # (the planted scenes keep every dot product far from 0)
    assert [k != NO_KEY for k in keys] == [k != NO_KEY for k in ref["keys"]], name
    for vtx, u in enumerate(targets):
        assert (u == -1) == (keys[vtx] == NO_KEY)
        if u >= 0:
            assert not ref["i64"][vtx][u]["why"], (name, vtx, u)
    return ref, keys, targets


def test_a_tetrahedron_has_nothing_to_remove():
    v, f, c = scene("tetrahedron")
    _, keys, targets = assert_proposals_are_the_restatements("tetrahedron")
    assert keys == [NO_KEY] * 4 and targets == [-1] * 4
    ov, of, oc, st = MD.decimate_mesh(v, f, c, 2)
    assert torch.equal(ov.cpu(), v) and torch.equal(of.cpu().long(), f) and torch.equal(oc.cpu(), c)
    assert not st["reached"] and st["stopped"] == "no valid collapse" and st["rounds"] == 0 and st["faces_after"] == 4 and st["accepted"] == []


def test_an_octahedron_goes_down_to_a_tetrahedron():
    v, f, c = scene("octahedron")
    ref, keys, targets = assert_proposals_are_the_restatements("octahedron")
    assert all(k != NO_KEY for k in keys) and targets == ref["targets"]
    ov, of, oc, st = MD.decimate_mesh(v, f, c, 0)
    rep = Dm.manifold_report(of.cpu().numpy(), ov.shape[0])
    assert st["accepted"] == [1, 1] and st["faces_after"] == 4 and not st["reached"] and st["stopped"] == "no valid collapse"
    assert rep == {"edges_twice_opposite": True, "euler": 2, "duplicates": 0, "degenerate": 0, "used_vertices": 4} and ov.shape[0] == 4
    kept, faces, rst = Dm.decimate(v, f, 0)
    assert np.array_equal(faces, of.cpu().numpy()) and torch.equal(ov.cpu(), v[kept]) and rst["accepted"] == st["accepted"]


def test_an_open_grid_keeps_its_rim():
    v, f, c = scene("grid")
    rim = Dm.grid_rim()
    _, keys, targets = assert_proposals_are_the_restatements("grid")
    assert all((k == NO_KEY) == bool(r) for k, r in zip(keys, rim.tolist()))            # no vertex on the open edge proposes; the interior does
    ov, of, oc, st = MD.decimate_mesh(v, f, c, 0)
    nrim = int(rim.sum())
    assert st["boundary_vertices_before"] == nrim == st["boundary_vertices_after"] and not st["reached"] and st["stopped"] == "no valid collapse"
    rows = {tuple(r) for r in ov.cpu().tolist()}
    assert all(tuple(r) in rows for r in v[rim].tolist())                                # every rim vertex is still there, bit for bit
    und, cnt, _ = R.undirected_counts(of.cpu().numpy())
    assert int((cnt == 1).sum()) == nrim and int((cnt > 2).sum()) == 0                   # the same open edges, nothing non-manifold
    print(f"open grid: {f.shape[0]} -> {st['faces_after']} faces in {st['rounds']} rounds, {ov.shape[0]} vertices of which {nrim} on the rim")


def test_the_valence_cap_holds_on_both_ends():
    # the apexes of the two fans are above the cap and never propose; no rim vertex goes to one
    v, f, c = scene("bipyramid")
    _, keys, targets = assert_proposals_are_the_restatements("bipyramid")
    assert keys[0] == keys[1] == NO_KEY and all(k != NO_KEY for k in keys[2:]) and all(u >= 2 for u in targets[2:])
    ov, of, oc, st = MD.decimate_mesh(v, f, c, Dm.FAN - 2 * 12)
    assert st["reached"] and st["faces_after"] == Dm.FAN - 24 and torch.equal(ov[:2].cpu(), v[:2])
    faces = of.cpu()
    assert int((faces == 0).any(1).sum()) == int((faces == 1).any(1).sum()) == (Dm.FAN - 24) // 2          # the apexes only ever lost faces
    # the cap on the target alone, on the 320-face icosphere: nothing under 6, only 5 <-> 6 under 7 (tests/test_mesh_decimate_cpu.py)
    size = [len(s) for s in Dm.stars(restated("ico2")["faces"], scene("ico2")[0].shape[0])]
    for cap, want in ((6, set()), (7, {(5, 6), (6, 5)})):
        _, keys, targets = assert_proposals_are_the_restatements("ico2", cap)
        assert {(size[vtx], size[u]) for vtx, u in enumerate(targets) if u >= 0} == want


def test_a_collapse_that_would_flip_a_face_is_refused():
    d = Dm.DART
    ref, keys, targets = assert_proposals_are_the_restatements("dart")
    assert targets == ref["targets"] == [d["notch"], -1, -1, -1, -1] and keys[0] == ref["keys"][0]
    assert ref["i64"][0][d["left"]]["why"] == {"flip"} == ref["i64"][0][d["right"]]["why"]


def test_unreferenced_vertices_are_left_alone():
    v, f, c = scene("unreferenced")
    ref, keys, targets = assert_proposals_are_the_restatements("unreferenced")
    used = torch.zeros(v.shape[0], dtype=torch.bool)
    used[f.reshape(-1)] = True
    loose = torch.nonzero(~used).reshape(-1).tolist()
    assert len(loose) == 5 and all(keys[i] == NO_KEY for i in loose) and all(k != NO_KEY for i, k in enumerate(keys) if i not in loose)
    ov, of, oc, st = MD.decimate_mesh(v, f, c, 100)
    rows = [tuple(r) for r in ov.cpu().tolist()]
    assert st["reached"] and all(tuple(r) in rows for r in v[~used].tolist()) and ov.shape[0] == v.shape[0] - sum(st["accepted"])


# ---- 3. selection -------------------------------------------------------------------------------------------------------------------------
def graph_distance_at_least_3(faces, V, chosen):
    nbr = Dm.neighbours(Dm.stars(faces, V))
    for a in chosen:
        near = set(nbr[a])
        for x in nbr[a]:
            near |= nbr[x]
        if (near - {a}) & set(chosen):
            return False
    return True


@pytest.mark.parametrize("name", ("flat", "noisy"))
def test_selection_is_the_restatements_on_the_kernels_keys(name):
    v, f, _ = scene(name)
    V = v.shape[0]
    ref = restated(name)
    _, keys_t, keys, targets = kernel_round(name)
    accept, flags = MD.select(f, V, keys_t)
    accept = accept.cpu().tolist()
    chosen = [i for i, a in enumerate(accept) if a]
    assert accept == Dm.select(ref["faces"], keys) and flags == (True, True) and chosen
    assert graph_distance_at_least_3(ref["faces"], V, chosen)
    assert all(keys[i] != NO_KEY and not ref["i64"][i][targets[i]]["why"] for i in chosen)
    assert len({targets[i] for i in chosen}) == len(chosen) and not {targets[i] for i in chosen} & set(chosen)
    if name == "flat":                                                  # every cost is 0: the index alone decides
        assert all(k == NO_KEY or k == i for i, k in enumerate(keys)) and chosen[0] == min(i for i, k in enumerate(keys) if k != NO_KEY)
    else:                                                               # a limit between the accepted costs keeps the cheaper ones
        costs = sorted(Dm.bits_cost(keys[i] >> 32) for i in chosen)
        limit = costs[len(costs) // 2]
        part, pflags = MD.select(f, V, keys_t, max_error=limit)
        assert part.cpu().tolist() == Dm.select(ref["faces"], keys, Dm.cost_bits(limit)) and pflags == (True, True)
        assert 0 < int(part.sum()) == sum(c <= limit for c in costs) < len(chosen)
        none, nflags = MD.select(f, V, keys_t, max_error=0.5 * costs[0])
        assert not none.any() and nflags == (True, False)               # the cheapest key costs more than the limit
    print(f"{name}: {len(chosen)} of {V} vertices accepted")


# ---- 4. the last round's cut ----------------------------------------------------------------------------------------------------------------
def test_the_cut_keeps_the_cheapest_proposals():
    v, f, c = scene("ico3")
    V, F = v.shape[0], f.shape[0]
    ref = restated("ico3")
    _, keys_t, keys, targets = kernel_round("ico3")
    accept, _ = MD.select(f, V, keys_t)
    n = int(accept.sum())
    assert n >= 8
    for target, keep in ((F - 2 * 5, 5), (F - 2 * 5 + 1, 5), (F - 1, 1), (F, 0), (F + 3, 0), (F - 2 * n, n), (0, n)):
        out = MD.cut(keys_t, accept, F, target).cpu().tolist()
        assert out == Dm.cut(keys, accept.cpu().tolist(), F, target) and sum(out) == keep, target
        kept = sorted(keys[i] for i, a in enumerate(out) if a)
        assert kept == sorted(keys[i] for i, a in enumerate(accept.cpu().tolist()) if a)[:keep]
    # a target inside the first round, even and odd: exactly the target, or one less
    for target in (F - 2 * 5, F - 2 * 5 + 1):
        ov, of, oc, st = MD.decimate_mesh(v, f, c, target)
        assert st["accepted"] == [5] and st["rounds"] == 1 and st["reached"] and of.shape[0] == F - 10 and ov.shape[0] == V - 5
        cheapest = sorted((keys[i], i) for i, a in enumerate(accept.cpu().tolist()) if a)[:5]
        gone = sorted(i for _, i in cheapest)
        assert torch.equal(ov.cpu(), v[[i for i in range(V) if i not in gone]])
        assert st["max_cost"] == Dm.bits_cost(cheapest[-1][0] >> 32)


# ---- 5. apply -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ico3", "noisy", "grid"))
def test_apply_is_exact_against_the_restatement(name):
    v, f, _ = scene(name)
    V = v.shape[0]
    ref = restated(name)
    Q, keys_t, keys, targets = kernel_round(name)
    accept, _ = MD.select(f, V, keys_t)
    faces, live, Q1 = MD.apply(f, V, accept, torch.tensor(targets), Q)
    want_faces, want_Q = Dm.apply(ref["faces"], accept.cpu().tolist(), targets, Q.numpy())
    alive = [t is not None for t in want_faces]
    assert live.cpu().tolist() == [int(a) for a in alive] and int(live.sum()) == f.shape[0] - 2 * int(accept.sum())
    got = faces.cpu().tolist()
    assert all((tuple(g) == w) if w is not None else (g == [V, V, V]) for g, w in zip(got, want_faces))
    assert np.array_equal(Q1.cpu().numpy(), want_Q) and not torch.equal(Q1.cpu(), Q)
    und, cnt, direction = R.undirected_counts(np.asarray([w for w in want_faces if w is not None]))
    if name != "grid":
        assert bool((cnt == 2).all() and (direction == 0).all())         # still closed after the round


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_loop(name):
    v, f, _ = scene(name)
    kept, faces, st = Dm.decimate(v, f, Dm.LOOP_CASES[name])
    return kept, faces, st, Dm.sphere_measures(v.numpy()[kept], faces, v, f)


@pytest.mark.parametrize("name", tuple(Dm.LOOP_CASES))
def test_decimation_end_to_end(name):
    v, f, c = scene(name)
    target = Dm.LOOP_CASES[name]
    ov, of, oc, st = MD.decimate_mesh(v, f, c, target)
    faces = of.cpu().numpy()
    rep = Dm.manifold_report(faces, ov.shape[0])
    assert rep == {"edges_twice_opposite": True, "euler": 2, "duplicates": 0, "degenerate": 0, "used_vertices": ov.shape[0]}
    assert of.shape[0] in (target, target - 1) and st["reached"] and st["stopped"] == "target" and st["faces_after"] == of.shape[0]
    assert st["rounds"] == len(st["accepted"]) > MD.ROUND_GROUP and 2 * sum(st["accepted"]) == f.shape[0] - of.shape[0]
    assert st["boundary_vertices_before"] == 0 == st["boundary_vertices_after"] and st["vertices_after"] == ov.shape[0] == v.shape[0] - sum(st["accepted"])
    json.loads(json.dumps(st, allow_nan=False))
    # a bit-equal subset of the input's vertices and colours, in their order
    index = {tuple(r): i for i, r in enumerate(v.tolist())}
    assert len(index) == v.shape[0]
    kept = [index[tuple(r)] for r in ov.cpu().tolist()]
    assert kept == sorted(kept) and torch.equal(ov.cpu(), v[kept]) and torch.equal(oc.cpu(), c[kept])
    # two runs are bit-equal
    ov2, of2, oc2, st2 = MD.decimate_mesh(v, f, c, target)
    assert torch.equal(ov2, ov) and torch.equal(of2, of) and torch.equal(oc2, oc) and st2 == st
    # closed from 4 cameras, and culling the back faces changes nothing
    cams = D.cams_for(64, 64, n=4, elevation=15.0)
    bg = [1.0, 1.0, 1.0]
    frames = torch.stack([MR.render_mesh(cam, v, f, c, bg)["render"] for cam in cams])
    fid = MR.mesh_fidelity(ov, of, oc, cams, frames, bg)
    assert fid["odd_hit_pixels"] == [0, 0, 0, 0] and min(fid["coverage"]) > 0.05
    for cam in cams:
        on, off = MR.render_mesh(cam, ov, of, oc, bg, cull=True), MR.render_mesh(cam, ov, of, oc, bg, cull=False)
        assert torch.equal(on["render"], off["render"]) and torch.equal(on["face_id"], off["face_id"])
    # as near the sphere as the restatement's result, up to the freedom of picking another collapse among costs within rounding
    _, rfaces, rst, want = restated_loop(name)
    meas = Dm.sphere_measures(ov.cpu().numpy(), faces, v, f)
    same = np.array_equal(rfaces, faces)
    ratios = {"radial_ratio": meas["radial"] / want["radial"], "volume_error_ratio": abs(meas["volume_ratio"] - 1) / abs(want["volume_ratio"] - 1)}
    print(f"{name}: {f.shape[0]} -> {of.shape[0]} faces in {st['rounds']} rounds (restatement {rst['rounds']}), largest cost {st['max_cost']:.3e}; "
          f"radial {meas['radial']:.4e} (restatement {want['radial']:.4e}), volume ratio {meas['volume_ratio']:.6f} ({want['volume_ratio']:.6f}); "
          f"faces equal to the restatement's: {same}; PSNR against the input's render {fid['psnr_mean']:.2f} dB")
    record_parity(f"mesh_decimate_end_to_end[{name}]", {"faces_before": int(f.shape[0]), "faces_after": int(of.shape[0]), "rounds": st["rounds"],
                                                        "rounds_restatement": rst["rounds"], "max_cost": st["max_cost"], **meas, **ratios,
                                                        "faces_equal_restatement": bool(same), "psnr_mean": fid["psnr_mean"]})
    assert meas["radial"] <= 2 * want["radial"] and abs(meas["volume_ratio"] - 1) <= 2 * abs(want["volume_ratio"] - 1)


def test_max_error_and_the_round_cap_stop_a_run():
    v, f, c = scene("ico3")
    full = MD.decimate_mesh(v, f, c, 200)[3]
    limit = sorted([full["max_cost"] * 0.25, 1e-7])[1]
    ov, of, oc, st = MD.decimate_mesh(v, f, c, 200, max_error=limit)
    assert not st["reached"] and st["stopped"] == "max_error" and 200 < st["faces_after"] < f.shape[0] and 0 < st["max_cost"] <= limit
    again = MD.decimate_mesh(v, f, c, 200, max_error=limit)
    assert torch.equal(again[1], of) and again[3] == st
    with pytest.raises(RuntimeError, match="after 3 rounds"):
        MD.decimate_mesh(v, f, c, 200, max_rounds=3)


# ---- 7. the script, chained -------------------------------------------------------------------------------------------------------------------
def test_decimate_mesh_script_end_to_end(tmp_path):
    v, f, c = scene("extracted")
    ply, out = str(tmp_path / "mesh.ply"), str(tmp_path / "mesh_small.ply")
    G.save_mesh_ply(ply, v, f, c)
    rv, rf, rc8 = G.read_mesh_ply(ply)
    video = str(tmp_path / "orbit.npy")
    from v3d_amd.recon.mesh_render import render_mesh_orbit
    np.save(video, render_mesh_orbit(rv, rf, rc8.astype(np.float32) / 255.0, 2, 2.0, 0.0, 60.0, 64, True))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pub", "decimate_mesh.py"), "--mesh", ply, "-o", out, "--target_faces", "400",
                        "--render_orbit", "2", "-w", "--video", video], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "400 triangles" in r.stdout and "before: PSNR mean" in r.stdout and "after:  PSNR mean" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["mesh.ply", "mesh_small.json", "mesh_small.ply", "mesh_small_orbit", "orbit.npy"]
    assert sorted(os.listdir(tmp_path / "mesh_small_orbit")) == ["000.png", "001.png", "orbit.npy"]
    stats = json.load(open(tmp_path / "mesh_small.json"))
    assert stats["faces_before"] == f.shape[0] and stats["faces_after"] == 400 and stats["reached"] and stats["stopped"] == "target"
    assert stats["fidelity_after"]["odd_hit_pixels"] == [0, 0] == stats["fidelity_before"]["odd_hit_pixels"] and stats["fidelity_before"]["psnr_mean"] > stats["fidelity_after"]["psnr_mean"] > 20
    ov, of, oc, st = MD.decimate_mesh(rv, rf, rc8.astype(np.float32) / 255.0, 400)
    dv, df, dc = G.read_mesh_ply(out)
    assert np.array_equal(dv, ov.cpu().numpy()) and np.array_equal(df, of.cpu().numpy()) and np.array_equal(dc, rc8[[int(i) for i in _rows(rv, dv)]])
    # render_mesh.py and clean_mesh.py take the output unchanged (in this process: the script under test above ran in its own)
    orbit = str(tmp_path / "orbit")
    _entry("render_mesh").main(["--mesh", out, "-o", orbit, "--render_orbit", "1", "--reso", "32", "-w"])
    assert sorted(os.listdir(orbit)) == ["000.png", "orbit.npy"]
    clean = str(tmp_path / "clean.ply")
    _entry("clean_mesh").main(["--mesh", out, "-o", clean, "--smooth", "2"])
    cs = json.load(open(tmp_path / "clean.json"))
    assert cs["faces"] == 400 and cs["vertices"] == dv.shape[0] and len(cs["components_after"]) == 1 and cs["boundary_vertices_after"] == 0


def _rows(before, after):
    index = {tuple(r): i for i, r in enumerate(np.asarray(before).tolist())}
    return [index[tuple(r)] for r in np.asarray(after).tolist()]


# ---- 8. nothing to do -----------------------------------------------------------------------------------------------------------------------
def test_empties_and_targets_that_ask_for_nothing_on_the_device():
    v, f, c = scene("ico2")
    none = torch.zeros(0, 3, dtype=torch.int64)
    for vv, ff, cc, target in ((v, none, c, 0), (v[:0], none, c[:0], 7), (v, f, c, f.shape[0]), (v, f, c, f.shape[0] + 1)):
        ov, of, oc, st = MD.decimate_mesh(vv, ff, cc, target)
        assert ov.is_cuda and torch.equal(ov.cpu(), vv) and torch.equal(of.cpu().long(), ff) and torch.equal(oc.cpu(), cc)
        assert st["rounds"] == 0 and st["reached"] and st["faces_after"] == ff.shape[0]
    Q = MD.vertex_quadrics(v, none)
    assert Q.is_cuda and not Q.any() and MD.propose(v, none, Q)[0].tolist() == [-1] * v.shape[0]
    ov, of, oc, st = MD.decimate_mesh(v, f, c, f.shape[0] - 1)          # one collapse: the smallest request that does something
    assert of.shape[0] == f.shape[0] - 2 and st["accepted"] == [1] and ov.shape[0] == v.shape[0] - 1
