"""The gfx950 mesh repair (csrc_recon/meshrepair.hip, v3d_amd/recon/mesh_repair.py, scripts/pub/repair_mesh.py) against the restatement
(tests/mesh_repair_ref.py).  Every raw entry is fed the restated inputs of its pass (the restated census and pair counts: no float decision
stands between the two) and must return the restated outputs exactly, new vertices bit for bit, into guarded buffers, twice alike.  The
whole loop must return the restatement's mesh, history and report on every scene that tests/test_mesh_repair_cpu.py holds to SCENE_MARGIN in
every round; of the scenes that do not keep it only the weaker statements are asked."""
import importlib.util
import json
import os
import time

import numpy as np
import pytest
import torch

import mesh_check_ref as R
import mesh_render_ref as M
import mesh_repair_ref as P
from conftest import record_parity
from v3d_amd.ops import get_ops
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_check as MK
from v3d_amd.recon import mesh_clean as MC
from v3d_amd.recon import mesh_decimate as MD
from v3d_amd.recon import mesh_repair as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096


class Guarded:
    """An output of n rows with GUARD sentinel elements before and after it (the pattern of tests/test_mesh_check_gpu.py)"""

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


def ints(x, width=1):
    t = torch.tensor(np.asarray(x, dtype=np.int64).reshape(-1), dtype=torch.int32, device=DEV)
    return t.reshape(-1, width).contiguous() if width > 1 else t


def call(name, *args):
    lib = G.load_library()
    G._check(lib, getattr(lib, "v3d_recon_repair_" + name)(*args, G._stream()), name)


def out_i(n, width=1):
    return Guarded(n, width, torch.int32, -7)


def rows(t):
    return [tuple(r) for r in t.cpu().tolist()]


# ---- 1. the raw entries ---------------------------------------------------------------------------------------------------------------------
def run_passes(s, grow_times):
    """every entry on the restated inputs of its pass, outputs guarded, compared exactly;  returns the outputs for the two-runs check"""
    ops, got = get_ops(), []
    v = torch.from_numpy(s["verts"]).to(DEV).contiguous()
    c = torch.from_numpy(s["colors"]).to(DEV).contiguous()
    V = v.shape[0]
    # weld
    kz, kxy, vals = Guarded(V, 1, torch.int64, -7), Guarded(V, 1, torch.int64, -7), out_i(V)
    call("weld_keys", v.data_ptr(), V, kz.ptr, kxy.ptr, vals.ptr)
    kz, kxy, vals = kz.take(), kxy.take(), vals.take()
    assert vals.cpu().tolist() == list(range(V))
    _, by_z = ops.gs_radix_sort_pairs(kz, vals, 32)
    _, order = ops.gs_radix_sort_pairs(kxy[by_z.long()].contiguous(), by_z, 64)
    heads = out_i(V)
    call("weld_heads", v.data_ptr(), V, order.data_ptr(), heads.ptr)
    heads = heads.take()
    assert int(heads.sum()) == len(set(s["remap"]))
    offsets = ops.gs_scan(heads)
    first, remap = out_i(V), out_i(V)
    call("weld_first", order.data_ptr(), heads.data_ptr(), offsets.data_ptr(), V, first.ptr)
    first = first.take()
    call("weld_remap", order.data_ptr(), offsets.data_ptr(), first.data_ptr(), V, remap.ptr)
    remap = remap.take()
    assert remap.cpu().tolist() == s["remap"]
    f = ints(s["faces"], 3)
    fw = out_i(f.shape[0], 3)
    call("remap_faces", f.data_ptr(), f.shape[0], V, remap.data_ptr(), fw.ptr)
    fw = fw.take()
    assert rows(fw) == s["faces_welded"]
    # drop
    ranges, corners = MC._corner_lists(fw, V)
    drop = out_i(fw.shape[0])
    call("drop_flags", v.data_ptr(), V, fw.data_ptr(), fw.shape[0], ranges.data_ptr(), corners.data_ptr(), drop.ptr)
    drop = drop.take()
    assert drop.cpu().tolist() == s["drop"]
    assert rows(MR._keep_faces(fw, V, (drop == 0).to(torch.int32))) == s["faces_kept"]
    got += [remap, fw, drop]
    # orient
    f = ints(s["faces_kept"], 3)
    F = f.shape[0]
    ranges, corners = MC._corner_lists(f, V)
    same, opposite = ints(s["orient_same"]), ints(s["orient_opposite"])
    cur, rounds = 2 * torch.arange(F, dtype=torch.int32, device=DEV), 0
    while True:
        nxt, changed = out_i(F), Guarded(1, 1, torch.int32, 0)                        # (the caller clears the word: its guards are zeros too)
        call("orient_round", f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(), cur.data_ptr(), nxt.ptr, changed.ptr)
        cur, rounds = nxt.take(), rounds + 1
        if int(changed.take()) == 0 or rounds > F + 8:
            break
    assert cur.cpu().tolist() == s["labels"] and rounds == s["orient_rounds"]
    assert MR._orient_labels(f, V, ranges, corners, same, opposite)[1] == rounds
    non = Guarded(F, 1, torch.int32, 0)
    call("orient_conflicts", f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(), cur.data_ptr(), non.ptr)
    non = non.take()
    assert non.cpu().tolist() == s["nonorient"]
    fa = out_i(F, 3)
    call("orient_apply", f.data_ptr(), F, cur.data_ptr(), non.data_ptr(), None, fa.ptr)
    fa = fa.take()
    assert rows(fa) == s["faces_applied"]
    assert rows(MR._orient(v, f)[0]) == s["faces_oriented"]
    got += [cur, non, fa]
    # cut
    f = ints(s["faces_oriented"], 3)
    ranges, corners = MC._corner_lists(f, V)
    bad, nxt = out_i(V), out_i(V)
    same, opposite, flags, per_face = ints(s["same"]), ints(s["opposite"]), ints(s["flags"]), ints(s["per_face"])      # (held until the kernels ran)
    call("vertex_open", f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(), flags.data_ptr(), bad.ptr, nxt.ptr)
    bad, nxt = bad.take(), nxt.take()
    assert bad.cpu().tolist() == s["bad"] and nxt.cpu().tolist() == s["next"]
    marks = out_i(F)
    call("trouble", f.data_ptr(), F, V, per_face.data_ptr(), bad.data_ptr(), marks.ptr)
    marks = marks.take()
    assert marks.cpu().tolist() == s["trouble"]
    if bool(marks.any()):
        for _ in range(grow_times):
            grown = out_i(F)
            call("grow", f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, marks.data_ptr(), grown.ptr)
            marks = grown.take()
    assert marks.cpu().tolist() == s["grown"]
    got += [bad, nxt, marks]
    if "cut_same" not in s:
        assert not s["faces_cut"]
        return got
    assert rows(MR._keep_faces(f, V, (marks == 0).to(torch.int32))) == s["faces_cut"]
    # fill
    f = ints(s["faces_cut"], 3)
    F = f.shape[0]
    ranges, corners = MC._corner_lists(f, V)
    bad, nxt = out_i(V), out_i(V)
    same, opposite, flags = ints(s["cut_same"]), ints(s["cut_opposite"]), ints(s["cut_flags"])
    call("vertex_open", f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(), flags.data_ptr(), bad.ptr, nxt.ptr)
    bad, nxt = bad.take(), nxt.take()
    assert bad.cpu().tolist() == s["cut_bad"] and nxt.cpu().tolist() == s["cut_next"]
    got += fill_passes(v, c, bad, nxt, s["cap"], s)
    return got


def fill_passes(v, c, bad, nxt, cap, want):
    """the doubling, the flags and the emit on (bad, next), guarded, against want["loop_labels" ..]"""
    V = bad.shape[0]
    lab, jump = torch.arange(V, dtype=torch.int32, device=DEV), torch.where(bad != 0, torch.full_like(nxt, -1), nxt).contiguous()
    for _ in range(P.DOUBLING_ROUNDS):
        lab2, jump2 = out_i(V), out_i(V)
        call("loop_round", V, lab.data_ptr(), jump.data_ptr(), lab2.ptr, jump2.ptr)
        lab, jump = lab2.take(), jump2.take()
    assert lab.cpu().tolist() == want["loop_labels"] and jump.cpu().tolist() == want["loop_jump"]
    live = (jump >= 0) & (jump < V)
    keys = torch.where(live, lab, torch.full_like(lab, V)).to(torch.int64).contiguous()
    keys_s, members = get_ops().gs_radix_sort_pairs(keys, torch.arange(V, dtype=torch.int32, device=DEV), max(1, V.bit_length()))
    ranges = torch.empty(V, 2, dtype=torch.int32, device=DEV)
    lib = G.load_library()
    G._check(lib, lib.v3d_recon_mesh_vertex_ranges(keys_s.data_ptr(), V, V, ranges.data_ptr(), G._stream()), "vertex_ranges")
    state, length = out_i(V), out_i(V)
    call("loop_flags", V, nxt.data_ptr(), bad.data_ptr(), lab.data_ptr(), jump.data_ptr(), ranges.data_ptr(), members.data_ptr(), cap, state.ptr, length.ptr)
    state, length = state.take(), length.take()
    assert state.cpu().tolist() == want["state"] and length.cpu().tolist() == want["length"]
    ops = get_ops()
    fillable = state == 1
    face_off = ops.gs_scan(torch.where(fillable, torch.where(length == 3, torch.ones_like(length), length), torch.zeros_like(length)).contiguous())
    vert_off = ops.gs_scan((fillable & (length > 3)).to(torch.int32))
    nf, nv = int(face_off[-1]), int(vert_off[-1])
    assert nf == len(want["new_faces"]) and nv == len(want["new_verts"])
    # (with nothing to fill the host never calls the entry; one guarded row shows that it would write nothing)
    new_f, new_v, new_c = out_i(max(nf, 1), 3), Guarded(max(nv, 1), 3, torch.float32, -7.0), Guarded(max(nv, 1), 3, torch.float32, -7.0)
    call("fill_emit", v.data_ptr(), c.data_ptr(), V, nxt.data_ptr(), ranges.data_ptr(), members.data_ptr(), state.data_ptr(), length.data_ptr(),
         face_off.data_ptr(), vert_off.data_ptr(), max(nf, 1), nv, new_f.ptr, new_v.ptr, new_c.ptr)
    new_f, new_v, new_c = new_f.take(), new_v.take(), new_c.take()
    assert rows(new_f[:nf]) == want["new_faces"] and bool((new_f[nf:] == -7).all())
    assert new_v[:nv].cpu().numpy().tobytes() == np.asarray(want["new_verts"], dtype=np.float32).tobytes() and bool((new_v[nv:] == -7.0).all())
    assert new_c[:nv].cpu().numpy().tobytes() == np.asarray(want["new_colors"], dtype=np.float32).tobytes() and bool((new_c[nv:] == -7.0).all())
    return [lab, jump, state, length, new_f, new_v, new_c]


RAW_SCENES = (("fold-1", {"grow_times": 1}), ("fold-2", {"grow_times": 2}), ("star-12", {}), ("two-0_1", {}), ("soup", {}), ("mixed", {}), ("cases", {}),
              ("moebius", {}), ("fin", {}), ("bow_tie", {}), ("icosphere", {}), ("open_grid", {}), ("open_grid", {"max_hole_edges": 8}), ("pair-1", {}),
              ("single-1", {}))


@pytest.mark.parametrize("name,kw", RAW_SCENES, ids=[P.key_of(n, k) for n, k in RAW_SCENES])
def test_every_raw_entry_equals_the_restatement_of_its_pass(name, kw):
    s = P.stages(name, kw)
    V = s["verts"].shape[0]
    if name == "fold-1":
        assert V == 162 and V % 64 != 0 and s["state"].count(1) == 2                # not a multiple of the wave
    if name == "icosphere":
        assert s["state"] == [0] * V and s["new_faces"] == []                        # no open edge: fill writes nothing
    if name == "single-1":
        assert len(s["faces"]) == 1 and s["length"][0] == 3 and s["new_faces"] == [(2, 1, 0)]         # F = 1, and a loop of exactly 3
    a = run_passes(s, kw.get("grow_times", 1))
    b = run_passes(s, kw.get("grow_times", 1))
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), "two runs differ"


def test_loops_at_the_cap_one_past_it_and_interleaved():
    s = P.stages("star-12", {})
    V = s["verts"].shape[0]
    v, c = torch.from_numpy(s["verts"]).to(DEV), torch.from_numpy(s["colors"]).to(DEV)
    bad, nxt = ints(s["cut_bad"]), ints(s["cut_next"])
    assert max(s["length"]) == 6
    for cap, states in ((6, 1), (5, 2)):                                             # exactly max_hole_edges, and one longer
        state, length, members = P.loop_flags(s["cut_bad"], s["cut_next"], s["loop_labels"], s["loop_jump"], cap)
        assert sorted(set(state)) == [0, states]
        new_f, new_v, new_c = P.fill_emit(s["verts"], s["colors"], s["cut_next"], state, length, members)
        fill_passes(v, c, bad, nxt, cap, {**s, "state": state, "length": length, "new_faces": new_f, "new_verts": new_v, "new_colors": new_c})
    # two loops whose vertex ranges interleave, a dead end into a bad vertex, and a chain into a loop
    nxt = [2, 3, 4, 5, 0, 7, 8, 1, -1, 1] + [-1] * 60
    bad = [0] * 8 + [1] + [0] * 61
    lab, jump = P.loop_labels(bad, nxt)
    state, length, members = P.loop_flags(bad, nxt, lab, jump, 10)
    assert state[:2] == [1, 2] and members[1] == [1, 3, 5, 7, 9]
    nxt[9] = -1
    lab, jump = P.loop_labels(bad, nxt)
    state, length, members = P.loop_flags(bad, nxt, lab, jump, 10)
    assert state[:2] == [1, 1] and members == {0: [0, 2, 4], 1: [1, 3, 5, 7]}
    vv = torch.linspace(-1.0, 1.0, 210).reshape(70, 3).contiguous()
    new_f, new_v, new_c = P.fill_emit(vv.numpy(), vv.numpy()[::-1].copy(), nxt, state, length, members)
    fill_passes(vv.to(DEV), torch.from_numpy(vv.numpy()[::-1].copy()).to(DEV), ints(bad), ints(nxt), 10,
                {"loop_labels": lab, "loop_jump": jump, "state": state, "length": length, "new_faces": new_f, "new_verts": new_v, "new_colors": new_c})


def test_weld_by_value_and_drop_bits_by_hand():
    v = np.array([(0.0, 1.0, 2.0), (-0.0, 1.0, 2.0), (0.0, 1.0, np.float32(2.0) + np.float32(2.4e-7)), (0.0, 1.0, 2.0), (5.0, -0.0, 0.0), (5.0, 0.0, -0.0)],
                 dtype=np.float32)
    assert MR.weld_remap(v).cpu().tolist() == P.weld(v) == [0, 0, 2, 0, 4, 4]
    f = [(0, 2, 4), (4, 0, 2), (0, 0, 4), (0, 2, 9), (2, 4, 0), (0, 2, 2)]
    assert MR.drop_flags(v, np.asarray(f)).cpu().tolist() == P.drop_bits(v, f) == [0, 8, 6, 1, 8, 6]
    big = np.random.default_rng(3).integers(0, 4, size=(5000, 3)).astype(np.float32)   # 64 positions, 5000 vertices: long runs of equals
    assert MR.weld_remap(big).cpu().tolist() == P.weld(big)


# ---- 2. the whole loop ----------------------------------------------------------------------------------------------------------------------
def repaired(name, kw):
    v, f = P.named(name)
    args = {{"grow_times": "grow"}.get(k, k): x for k, x in kw.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = MR.repair_mesh(v, np.asarray(f), P.scene_colors(v.shape[0]), **args)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, (v, f)


def record(name, kw, info, faces_before, seconds):
    record_parity(f"mesh_repair_loop[{P.key_of(name, kw)}]", {"faces_before": faces_before, "faces_after": info["after"]["faces"], "rounds": len(info["history"]),
                                                              "pairs_before": info["before"]["self_intersections"],
                                                              "pairs_after": info["after"]["self_intersections"], "watertight": info["after"]["watertight"],
                                                              "stopped": info["stopped"], "seconds": seconds})


@pytest.mark.parametrize("name,kw", P.MARGIN_SCENES + P.PLAIN_SCENES, ids=[P.key_of(n, k) for n, k in P.MARGIN_SCENES + P.PLAIN_SCENES])
def test_repair_mesh_equals_the_restated_loop(name, kw):
    want = P.restated(name, kw)
    (v, f, c, info), seconds, (v0, f0) = repaired(name, kw)
    print(f"{P.key_of(name, kw)}: {len(f0)} -> {f.shape[0]} faces in {len(info['history'])} rounds ({info['stopped']}), {seconds:.3f} s")
    record(name, kw, info, len(f0), seconds)
    assert f.dtype == torch.int32 and rows(f) == want["faces"]
    assert v.cpu().numpy().tobytes() == want["verts"].tobytes() and c.cpu().numpy().tobytes() == want["colors"].tobytes()
    assert info["history"] == want["history"] and info["stopped"] == want["stopped"] and info["orient"] == want["orient"]
    assert info["loops_left"] == want["loops_left"]
    before = P.report(v0, f0)
    if "soup" in name:                                                             # unwelded neighbours touch along whole edges: the pair rule stands at margin 0
        before = {k: x for k, x in before.items() if k not in ("self_intersections", "intersecting_faces", "watertight")}
    assert R.same_report(info["after"], want["after"]) and R.same_report(info["before"], before)
    assert MK.check_mesh(v, f)["watertight"] is want["after"]["watertight"]
    if name == "icosphere":                                                        # nothing to repair: bit-equal, no rounds
        assert info["history"] == [] and v.cpu().numpy().tobytes() == v0.tobytes() and rows(f) == f0
    again = MR.repair_mesh(v0, np.asarray(f0), P.scene_colors(v0.shape[0]), **{{"grow_times": "grow"}.get(k, k): x for k, x in kw.items()})
    assert torch.equal(again[0], v) and torch.equal(again[1], f) and torch.equal(again[2], c) and again[3]["history"] == info["history"], "two runs differ"


@pytest.mark.parametrize("name,kw", P.WEAK_SCENES, ids=[P.key_of(n, k) for n, k in P.WEAK_SCENES])
def test_scenes_without_the_margin_are_self_consistent(name, kw):
    """Their decisions may fall either way in float32: only what holds of any outcome is asked"""
    (v, f, c, info), seconds, (v0, f0) = repaired(name, kw)
    print(f"{P.key_of(name, kw)}: {len(f0)} -> {f.shape[0]} faces in {len(info['history'])} rounds ({info['stopped']}), {seconds:.3f} s; {info['history']}")
    record(name, kw, info, len(f0), seconds)
    assert R.same_report(info["after"], P.report(v.cpu().numpy(), rows(f)))
    faces = None
    for h in info["history"]:
        assert set(h) == set(MR.HISTORY_KEYS) and (faces is None or h["faces"] == faces)
        assert h["faces_after"] == h["faces"] - h["faces_cut"] + h["faces_filled"] - h["faces_dropped"]
        faces = h["faces_after"]
    assert faces is None or faces == f.shape[0] and c.shape == v.shape


def test_the_output_of_the_decimation_goes_through():
    """Not a promise about decimate_mesh or about this stage: whatever comes back, the kernels and the restatement say the same of it"""
    v, f = M.icosphere(3, 0.5, (0.0, 0.0, 0.0), 1)
    dv, df, _, _ = MD.decimate_mesh(v, f, None, 400)
    rv, rf, rc, info = MR.repair_mesh(dv, df)
    print(f"decimated 1280 -> {df.shape[0]} -> repaired {rf.shape[0]} faces: {info['history']}; {info['after']}")
    assert rc is None and R.same_report(info["after"], P.report(rv.cpu().numpy(), rows(rf)))
    record_parity("mesh_repair_downstream[decimate-1280-400]", {"faces_before": int(df.shape[0]), "faces_after": int(rf.shape[0]), "rounds": len(info["history"]),
                                                                "pairs_before": info["before"]["self_intersections"],
                                                                "pairs_after": info["after"]["self_intersections"], "watertight": info["after"]["watertight"]})


# ---- 3. the script --------------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_repair_mesh_script_end_to_end(tmp_path, capsys):
    mod = _entry("repair_mesh")
    v, f = P.named("fold-1")
    colors = np.rint(P.scene_colors(v.shape[0]) * 255.0).astype(np.float32) / 255.0   # what a PLY can hold
    src, out, rep = str(tmp_path / "fold.ply"), str(tmp_path / "fold_repaired.ply"), str(tmp_path / "fold_repair.json")
    G.save_mesh_ply(src, v, np.asarray(f), colors)
    mod.main(["--mesh", src, "-o", out, "--json", rep, "--strict"])                  # repaired: status 0 under --strict
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3 and "NOT watertight" in lines[0] and "69 intersecting pairs" in lines[0] and ": watertight; 264 triangles" in lines[1]
    want = P.repair(v, f, colors)
    pv, pf, pc = G.read_mesh_ply(out)
    assert pv.tobytes() == want["verts"].tobytes() and [tuple(r) for r in pf.tolist()] == want["faces"]
    assert np.array_equal(pc, np.rint(np.clip(want["colors"], 0, 1) * 255.0).astype(np.uint8))                 # the colours came along
    r = json.load(open(rep))
    assert r["mesh"] == src and r["out"] == out and r["history"] == want["history"] and R.same_report(r["after"], want["after"]) and r["after"]["watertight"]
    # an unrepaired mesh under --strict: status 1, and the file is written all the same
    gv, gf = P.named("open_grid")
    grid, grid_out = str(tmp_path / "grid.ply"), str(tmp_path / "grid_out.ply")
    G.save_mesh_ply(grid, gv, np.asarray(gf), P.scene_colors(gv.shape[0]))
    with pytest.raises(SystemExit) as e:
        mod.main(["--mesh", grid, "-o", grid_out, "--max_hole_edges", "8", "--strict"])
    assert e.value.code == 1 and G.read_mesh_ply(grid_out)[1].shape[0] == 30
    mod.main(["--mesh", grid, "-o", grid_out, "--max_hole_edges", "8"])              # a plain run exits 0 whatever is left
    # nothing but faces that are none: an empty result is refused and nothing is written
    flat, flat_out = str(tmp_path / "flat.ply"), str(tmp_path / "flat_out.ply")
    G.save_mesh_ply(flat, gv, np.asarray([(0, 0, 1), (2, 2, 2)]), P.scene_colors(gv.shape[0]))
    with pytest.raises(SystemExit) as e:
        mod.main(["--mesh", flat, "-o", flat_out])
    assert e.value.code not in (0, 1, None) and "nothing" in str(e.value.code) and not os.path.exists(flat_out)
