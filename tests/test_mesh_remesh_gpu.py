"""The gfx950 remeshing (csrc_recon/meshremesh.hip, v3d_amd/recon/mesh_remesh.py, scripts/pub/remesh_mesh.py) against the restatement
(tests/mesh_remesh_ref.py): every propose entry on every case, the selection on the kernel's own keys, every apply entry on the kernel's own
accepted set, the relaxation and the reprojection, whole runs, the entry point chained into the other mesh scripts, and the empty cases.

Decisions (who proposes what with which key, who is accepted, which faces are written, which rows are appended, the counts) are exact against
the float32 restatement, which runs the kernels' own arithmetic; a vertex is left out where the fp64 restatement comes within 1e-6, relative,
of a threshold, and at most 2 % of a case's vertices may be.  Floats follow the rule of tests/test_mesh_clean_gpu.py: the kernel may be off
from the fp64 restatement by 4x what the restatement's own float32 run is off (mesh_clean_ref.float_bar).  4096 sentinels stand on either
side of every output.  The figures go to the parity record."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_decimate_ref as Dm
import mesh_remesh_ref as Rm
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_decimate as MD
from v3d_amd.recon import mesh_remesh as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_KEY = Rm.NO_KEY
SENT = 4096
MARK = {torch.int32: -77777, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.float32: 1234.5}
CLOSED = {"edges_twice_opposite": True, "euler": 2, "duplicates": 0, "degenerate": 0}
OPS = ("split", "collapse", "flip")


def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- guarded buffers --------------------------------------------------------------------------------------------------------------------------
def guarded(shape, dtype, init=None):
    """(buffer, view): `view` of `shape` in the middle of a buffer with SENT marks on either side; the view starts as `init` or as marks"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * SENT,), MARK[dtype], dtype=dtype, device=DEV)
    view = buf[SENT:SENT + n].view(*shape)
    if init is not None:
        view.copy_(init)
    return buf, view


def intact(buf):
    m = MARK[buf.dtype]
    return bool((buf[:SENT] == m).all()) and bool((buf[-SENT:] == m).all())


class Guarded(MR.RemeshState):
    """A state whose verts, colors, faces, counts and removed stand between sentinels"""

    def __init__(self, name):
        v, f, c, self.L = Rm.case(name)
        super().__init__(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV).to(torch.int32), torch.from_numpy(c).to(DEV), Rm.SPARE)
        self.bufs = {}
        for key in ("verts", "colors", "faces", "counts", "removed"):
            t = getattr(self, key)
            self.bufs[key], view = guarded(tuple(t.shape), t.dtype, t)
            setattr(self, key, view)

    def intact(self):
        return all(intact(b) for b in self.bufs.values())


def propose(st, op, L):
    """(keys, targets) of the entry itself, written between sentinels"""
    lib = G.load_library()
    kb, keys = guarded((st.Vcap,), torch.int64)
    tb, targets = guarded((st.Vcap,), torch.int32)
    ranges, corners = st.lists()
    head = (st.verts.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, ranges.data_ptr(), corners.data_ptr())
    tail = (Rm.DEFAULT_MAX_VALENCE, keys.data_ptr(), targets.data_ptr(), G._stream())
    if op == "flip":
        rc = lib.v3d_recon_remesh_flip_propose(*head, MR.boundary(st).data_ptr(), *tail)
    else:
        rc = getattr(lib, f"v3d_recon_remesh_{op}_propose")(*head, L, *tail)
    G._check(lib, rc, op)
    torch.cuda.synchronize()
    assert intact(kb) and intact(tb), op
    return keys, targets


def unsigned(keys):
    return [k & NO_KEY for k in keys.tolist()]


def expected_faces(raw, first, after, Vcap):
    """The face array the kernel must hold: the restatement's faces, Vcap Vcap Vcap for a face that died, the raw row for one never present"""
    out = np.full((len(after), 3), Vcap, dtype=np.int64)
    out[:raw.shape[0]] = raw
    for i, tri in enumerate(after):
        if tri is not None:
            out[i] = tri
        elif first[i] is not None:
            out[i] = Vcap
    return out


def rows32(rows):
    return np.array(rows, dtype=np.float32).reshape(-1, 3)


# ---- 1. every operation on every case -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(Rm.CASES))
def test_propose_select_and_apply_are_the_restatements(name):
    v, f, c, L = Rm.case(name)
    figures = {}
    for op in OPS:
        st = Guarded(name)
        keys_t, targets_t = propose(st, op, L)
        keys, targets = unsigned(keys_t), targets_t.tolist()
        ref, k32, t32, _ = Rm.proposals(name, op, np.float32)
        _, _, _, margin = Rm.proposals(name, op)
        out = Rm.excluded(margin)
        assert sum(out) <= Rm.EXCLUDE_MAX * len(out), (name, op)
        assert len(keys) == ref.Vcap == st.Vcap
        for i, skip in enumerate(out):
            if not skip:
                assert keys[i] == k32[i] and targets[i] == t32[i], (name, op, i, hex(keys[i]), hex(k32[i]), targets[i], t32[i])
        n_prop = sum(k != NO_KEY for k in keys)
        # two runs are bit-equal
        again_k, again_t = propose(st, op, L)
        assert torch.equal(again_k, keys_t) and torch.equal(again_t, targets_t)
        # the selection, on the kernel's own keys
        accept_t, flags = MR.select(st, keys_t)
        accept = accept_t.tolist()
        assert accept == Dm.select(ref.faces, keys), (name, op)
        assert flags.tolist() == [int(any(accept))] * 2
        real = [k for k in keys if k != NO_KEY]
        assert len(set(real)) == len(real)
        # the apply entry, on the kernel's own accepted set
        first = list(ref.faces)
        lib = G.load_library()
        ranges, corners = st.lists()
        if op == "split":
            rank = MR.get_ops().gs_scan(accept_t)
            cb, counts = guarded((2,), torch.int32)
            fb, flag = guarded((1,), torch.int32, torch.zeros(1, dtype=torch.int32))
            G._check(lib, lib.v3d_recon_remesh_split_apply(st.verts.data_ptr(), st.colors.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, ranges.data_ptr(),
                                                           corners.data_ptr(), accept_t.data_ptr(), targets_t.data_ptr(), rank.data_ptr(),
                                                           st.counts.data_ptr(), counts.data_ptr(), flag.data_ptr(), G._stream()), "split_apply")
            torch.cuda.synchronize()
            Rm.split_apply(ref, accept, targets)
            assert intact(cb) and intact(fb) and counts.tolist() == [ref.V_live, ref.F_live] and flag.tolist() == [0] and not ref.flag
            assert ref.V_live == v.shape[0] + sum(accept) and rank.tolist()[-1] == sum(accept)
        elif op == "collapse":
            G._check(lib, lib.v3d_recon_remesh_collapse_apply(st.faces.data_ptr(), st.Fcap, st.Vcap, ranges.data_ptr(), corners.data_ptr(),
                                                              accept_t.data_ptr(), targets_t.data_ptr(), st.removed.data_ptr(), G._stream()), "collapse_apply")
            torch.cuda.synchronize()
            Rm.collapse_apply(ref, accept, targets)
            assert st.removed.tolist() == [int(x) for x in ref.removed] == accept
        else:
            G._check(lib, lib.v3d_recon_remesh_flip_apply(st.faces.data_ptr(), st.Fcap, st.Vcap, ranges.data_ptr(), corners.data_ptr(), accept_t.data_ptr(),
                                                          targets_t.data_ptr(), G._stream()), "flip_apply")
            torch.cuda.synchronize()
            before = Rm.potential(ref)
            Rm.flip_apply(ref, accept, targets)
            assert Rm.potential(ref) <= before - sum(accept)                 # every flip lowers the potential
        assert st.intact(), (name, op)
        assert np.array_equal(st.faces.cpu().numpy().astype(np.int64), expected_faces(f, first, ref.faces, st.Vcap)), (name, op)
        assert np.array_equal(st.verts.cpu().numpy().view(np.uint32), rows32(ref.P).view(np.uint32)), (name, op)
        assert np.array_equal(st.colors.cpu().numpy().view(np.uint32), rows32(ref.C).view(np.uint32)), (name, op)
        if op != "split":
            assert st.counts.tolist() == [v.shape[0], f.shape[0]]
        figures[op] = {"proposals": n_prop, "accepted": sum(accept), "excluded": sum(out)}
    print(f"{name}: {figures}")
    record_parity(f"mesh_remesh_operations[{name}]", {"vertices": int(v.shape[0]), "faces": int(f.shape[0]), "target_edge": L, **figures})
    if name in ("tetrahedron", "single", "dart"):
        assert figures["collapse"]["proposals"] == figures["flip"]["proposals"] == 0
    if name == "single":
        assert figures["split"]["proposals"] == 0
    if name == "bipyramid":
        assert figures["split"]["proposals"] == 350


@pytest.mark.parametrize("name", Rm.PLANTED)
def test_with_its_length_rules_open_wide_the_collapse_kernel_proposes_where_the_decimation_kernel_does(name):
    """The two propose kernels against each other (and the remeshing targets against the decimation restatement): the closed-fan walk and the
    integer rules are one piece of code, the normal tests are each kernel's own, and on these scenes no normal test is near its threshold"""
    v, f, c = Dm.scene(name)
    cap = Rm.DEFAULT_MAX_VALENCE
    decim_keys, _ = MD.propose(v, f, MD.vertex_quadrics(v, f), max_valence=cap)
    st = MR.RemeshState(v.to(DEV), f.to(DEV).to(torch.int32), c.to(DEV), 0)
    keys, targets = MR.collapse_propose(st, Rm.OPEN_WIDE, cap)
    Rm.assert_collapse_proposers_agree(name, unsigned(decim_keys), unsigned(keys), targets.tolist(), cap)
    print(f"{name}: {sum(k != NO_KEY for k in unsigned(keys))} of {v.shape[0]} vertices propose in both kernels")


def test_a_capacity_one_vertex_short_drops_by_rank_and_writes_nothing_past_it():
    name = "net400"
    v, f, c, L = Rm.case(name)
    full = Guarded(name)
    keys_t, targets_t = propose(full, "split", L)
    accept_t, _ = MR.select(full, keys_t)
    n = int(accept_t.sum())
    assert n >= 4
    short = MR.RemeshState(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV).to(torch.int32), torch.from_numpy(c).to(DEV), n - 1)
    bufs = {}
    for key in ("verts", "colors", "faces"):
        t = getattr(short, key)
        bufs[key], view = guarded(tuple(t.shape), t.dtype, t)
        setattr(short, key, view)
    # (the lists do not depend on the capacity but for the name of the extra vertex: the keys of the full state select the same vertices)
    k2, t2 = MR.split_propose(short, L)
    a2, _ = MR.select(short, k2)
    assert a2.tolist() == accept_t.tolist()[:v.shape[0]] + [0] * (n - 1) and t2.tolist()[:v.shape[0]] == targets_t.tolist()[:v.shape[0]]
    flag = MR.split_apply(short, a2, t2)
    torch.cuda.synchronize()
    assert all(intact(b) for b in bufs.values())
    assert flag.tolist() == [1] and short.counts.tolist() == [short.Vcap, short.Fcap] == [v.shape[0] + n - 1, f.shape[0] + 2 * (n - 1)]
    ref = Rm.State(v, f, c, n - 1, np.float32)
    first = list(ref.faces)
    Rm.split_apply(ref, a2.tolist(), t2.tolist())
    assert ref.flag and np.array_equal(short.faces.cpu().numpy().astype(np.int64), expected_faces(f, first, ref.faces, short.Vcap))
    assert np.array_equal(short.verts.cpu().numpy().view(np.uint32), rows32(ref.P).view(np.uint32))
    # the state grows and the dropped split goes through in the next round
    short.grow(16)
    assert bool((short.faces[f.shape[0] + 2 * (n - 1):] == short.Vcap).all()) and short.Vcap == v.shape[0] + n + 15
    k3, t3 = MR.split_propose(short, L)
    last = max(i for i, on in enumerate(accept_t.tolist()) if on)
    assert t3.tolist()[last] == targets_t.tolist()[last] and (k3.tolist()[last] & NO_KEY) == (keys_t.tolist()[last] & NO_KEY)


# ---- 2. relax and reproject -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("net400", "noisy", "grid", "degenerate", "unreferenced", "bad_indices", "single"))
def test_relax_keeps_the_standing_bar_and_pins_the_open_edges(name):
    v, f, c, L = Rm.case(name)
    lib = G.load_library()
    st = Guarded(name)
    ranges, corners = st.lists()
    flags = MR.boundary(st)
    pinned = torch.zeros(st.Vcap, dtype=torch.int32, device=DEV)
    pinned[::7] = 1
    ob, out = guarded((st.Vcap, 3), torch.float32)
    outs = []
    for pins in (None, pinned, None):
        G._check(lib, lib.v3d_recon_remesh_relax(st.verts.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, ranges.data_ptr(), corners.data_ptr(),
                                                 flags.data_ptr(), pins.data_ptr() if pins is not None else None, 0.5, out.data_ptr(), G._stream()), "relax")
        torch.cuda.synchronize()
        assert intact(ob) and st.intact()
        outs.append(out.cpu().clone())
    assert torch.equal(outs[0], outs[2])                                                     # two runs are bit-equal
    r64, r32 = Rm.State(v, f, c, Rm.SPARE), Rm.State(v, f, c, Rm.SPARE, np.float32)
    want64, want32 = torch.tensor(np.array(Rm.relax(r64, 0.5), dtype=np.float64)), torch.from_numpy(rows32(Rm.relax(r32, 0.5)))
    err, err32, bound = C.float_bar(outs[0], want64, want32)
    moved = int((outs[0] != st.verts.cpu()).any(1).sum())
    p64 = torch.tensor(np.array(Rm.relax(r64, 0.5, pinned=pinned.tolist()), dtype=np.float64))
    perr, _, pbound = C.float_bar(outs[1], p64, torch.from_numpy(rows32(Rm.relax(r32, 0.5, pinned=pinned.tolist()))))
    print(f"{name}: relax {err:.3e} from fp64 (float32 restatement {err32:.3e}, bound {bound:.3e}); pinned {perr:.3e} (bound {pbound:.3e}); {moved} moved")
    record_parity(f"mesh_remesh_relax[{name}]", {"max_abs": err, "float32_restatement": err32, "bound": bound, "pinned_max_abs": perr, "pinned_bound": pbound,
                                                 "moved": moved})
    assert err <= bound and perr <= pbound
    still = (flags.cpu() != 0) | (torch.tensor([len(s) == 0 for s in r64.stars()]))
    assert torch.equal(outs[0][still], st.verts.cpu()[still]) and torch.equal(outs[1][::7], st.verts.cpu()[::7])
    assert flags.cpu().tolist() == Rm.boundary_flags(r64.stars())
    if name == "grid":
        assert torch.equal(outs[0][:v.shape[0]][Dm.grid_rim()], torch.from_numpy(v)[Dm.grid_rim()]) and moved >= 0.99 * int((~Dm.grid_rim()).sum())
    if name == "single":
        assert moved == 0
    if name in ("net400", "noisy"):
        assert moved >= 0.99 * v.shape[0]
        # the step lies in the tangent plane: none of it along the vertex normal
        step = (outs[0][:v.shape[0]].double() - torch.from_numpy(v).double())
        normal = C.normals(torch.from_numpy(v), torch.from_numpy(f))
        assert float((step * normal).sum(1).abs().max()) < 1e-6 < float(step.norm(dim=1).max())


@pytest.mark.parametrize("name", ("net400", "grid", "ico3_200"))
def test_reprojection_lands_on_the_input_with_its_colours(name):
    from v3d_amd.recon.mesh_bake import build_bvh
    from v3d_amd.recon.mesh_query import closest_points
    v, f, c, L = Rm.case(name)
    tv, tf, tc = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV).to(torch.int32), torch.from_numpy(c).to(DEV)
    bvh = build_bvh(tv, tf, DEV)
    # the state to put back: one split round and one relaxation step away from the input
    st = Guarded(name)
    keys_t, targets_t = propose(st, "split", L)
    accept_t, _ = MR.select(st, keys_t)
    MR.split_apply(st, accept_t, targets_t)
    MR.relax_vertices(st, 0.5)
    start_v, start_c = st.verts.clone(), st.colors.clone()
    vb, verts = guarded((st.Vcap, 3), torch.float32, start_v)
    cb, cols = guarded((st.Vcap, 3), torch.float32, start_c)
    st.verts, st.colors = verts, cols
    _, face, uv = closest_points(bvh, start_v)
    MR.project_vertices(st, bvh, tc)
    torch.cuda.synchronize()
    assert intact(vb) and intact(cb)
    got_v, got_c = verts.cpu().clone(), cols.cpu().clone()
    # exact on the kernel's own closest points
    P32, C32 = [tuple(np.float32(x) for x in row) for row in start_v.cpu().tolist()], [tuple(np.float32(x) for x in row) for row in start_c.cpu().tolist()]
    eP, eC = Rm.project_rows(P32, C32, face.cpu().tolist(), uv.cpu().numpy().astype(np.float32), v, c, f, np.float32)
    assert np.array_equal(got_v.numpy().view(np.uint32), rows32(eP).view(np.uint32)) and np.array_equal(got_c.numpy().view(np.uint32), rows32(eC).view(np.uint32))
    # the whole, closest point included, against the restatement in both precisions
    refs = []
    for dt in (np.float64, np.float32):
        r = Rm.State(v, f, c, Rm.SPARE, dt)
        r.P = [tuple(r.T(x) for x in row) for row in start_v.cpu().tolist()]
        r.C = [tuple(r.T(x) for x in row) for row in start_c.cpu().tolist()]
        Rm.project(r, v, c, f)
        refs.append((torch.tensor(np.array(r.P, dtype=np.float64)), torch.tensor(np.array(r.C, dtype=np.float64))))
    live = int(st.counts[0])                      # (an unborn row lies at the origin: at a sphere's centre every face is as near as any other)
    err, err32, bound = C.float_bar(got_v[:live], refs[0][0][:live], refs[1][0][:live])
    cerr, cerr32, cbound = C.float_bar(got_c[:live], refs[0][1][:live], refs[1][1][:live])
    moved = int((got_v != start_v.cpu()).any(1).sum())
    print(f"{name}: reprojection {err:.3e} from fp64 (float32 restatement {err32:.3e}, bound {bound:.3e}); colours {cerr:.3e} ({cerr32:.3e}, bound "
          f"{cbound:.3e}); {moved} of {st.Vcap} rows moved, {int(accept_t.sum())} of them new")
    record_parity(f"mesh_remesh_project[{name}]", {"max_abs": err, "float32_restatement": err32, "bound": bound, "color_max_abs": cerr,
                                                   "color_float32_restatement": cerr32, "color_bound": cbound, "moved": moved})
    assert err <= bound and cerr <= cbound and int(accept_t.sum()) >= 1                      # (a round accepts vertices 3 edges apart: few)
    dist, _, _ = closest_points(bvh, verts)
    assert float(dist.max()) <= 2.0 ** -20                                                   # on the input surface
    # a miss keeps the vertex: the same call with every answer a miss
    lib = G.load_library()
    miss = torch.full_like(face, -1)
    G._check(lib, lib.v3d_recon_remesh_project(miss.data_ptr(), uv.data_ptr(), tv.data_ptr(), tc.data_ptr(), tv.shape[0], tf.data_ptr(), tf.shape[0],
                                               verts.data_ptr(), cols.data_ptr(), st.Vcap, G._stream()), "project")
    torch.cuda.synchronize()
    assert torch.equal(verts.cpu(), got_v) and torch.equal(cols.cpu(), got_c)


# ---- 3. whole runs --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_run(name):
    v, f, c = Rm.decimated(name)
    vo, fo, co, st = MR.remesh_mesh(v, f, c, iterations=3)
    return vo.cpu().numpy(), fo.cpu().numpy().astype(np.int64), co.cpu().numpy(), st


@pytest.mark.parametrize("name", tuple(Rm.LOOP_CASES))
def test_whole_runs_even_the_mesh_out_as_far_as_the_restatement_does(name):
    v, f, c = Rm.decimated(name)
    vo, fo, co, st = kernel_run(name)
    rv, rf, rc, rst = Rm.loop_run(name)
    assert Dm.manifold_report(fo, vo.shape[0]) == {**CLOSED, "used_vertices": vo.shape[0]}
    before, mine, want = Rm.measures(v, f), Rm.measures(vo, fo), Rm.measures(rv, rf)
    assert st["before"] == pytest.approx(before, rel=1e-9) and st["after"] == pytest.approx(mine, rel=1e-9)
    rd = Rm.Q.mesh_distance(torch.from_numpy(rv).float(), torch.from_numpy(rf), torch.from_numpy(v), torch.from_numpy(f))
    ref_far = rd["hausdorff"] / rd["diagonal"]
    print(f"{name}: {f.shape[0]} -> {fo.shape[0]} faces (restatement {rf.shape[0]}); operations {st['operations']} in rounds {st['rounds']} (restatement "
          f"{rst['ops']} in {rst['rounds']}); before {before}; after {mine}; restatement {want}; from the input {st['distance']['hausdorff']:.5f} of the "
          f"diagonal (restatement {ref_far:.5f}); {st['seconds']:.2f} s")
    record_parity(f"mesh_remesh_loop[{name}]", {"faces_before": int(f.shape[0]), "faces_after": int(fo.shape[0]), "restatement_faces": int(rf.shape[0]),
                                                "operations": st["operations"], "rounds": st["rounds"], "before": before, "after": mine,
                                                "restatement_after": want, "distance": st["distance"]["hausdorff"], "restatement_distance": ref_far,
                                                "seconds": st["seconds"]})
    for k, sign in Rm.MEASURES.items():
        assert (want[k] - before[k]) * sign > 0                                             # the restatement improves it ..
        assert (mine[k] - before[k]) * sign >= 0.5 * (want[k] - before[k]) * sign, k         # .. and the kernels at least half as far
    assert st["distance"]["hausdorff"] <= 2.0 * ref_far
    assert st["target_edge"] == rst["target_edge"] and st["reallocations"] == 0
    assert st["faces_after"] == fo.shape[0] and st["vertices_after"] == vo.shape[0] and co.shape == vo.shape
    json.loads(json.dumps(st, allow_nan=False))
    again = MR.remesh_mesh(v, f, c, iterations=3)                                           # two runs are bit-equal everywhere
    assert np.array_equal(again[0].cpu().numpy().view(np.uint32), vo.view(np.uint32)) and np.array_equal(again[1].cpu().numpy(), fo)
    assert np.array_equal(again[2].cpu().numpy().view(np.uint32), co.view(np.uint32))


def test_an_even_mesh_comes_back_with_its_faces():
    v, f, c = Dm.scene("ico3")
    vo, fo, co, st = MR.remesh_mesh(v, f, c, iterations=3)
    assert torch.equal(fo.cpu().long(), f) and all(n == [0, 0, 0] for n in st["operations"].values()) and vo.shape == v.shape


def _open_edges(v, f):
    und, cnt, _ = Dm.R.undirected_counts(np.asarray(f, dtype=np.int64))
    edges = np.asarray(und)[np.asarray(cnt) == 1]
    p = np.asarray(v, dtype=np.float32)
    return {p[i].tobytes() for i in np.unique(edges)}, {frozenset((p[a].tobytes(), p[b].tobytes())) for a, b in edges.tolist()}


def test_open_edges_stay_bit_for_bit():
    v, f, c, L = Rm.case("grid")
    vo, fo, co, st = MR.remesh_mesh(v, f, c, target_edge=L, iterations=3)
    vo, fo = vo.cpu().numpy(), fo.cpu().numpy().astype(np.int64)
    rim = Dm.grid_rim().numpy()
    assert _open_edges(v, f) == _open_edges(vo, fo) and len(_open_edges(v, f)[0]) == int(rim.sum())
    assert fo.shape[0] > 1.5 * f.shape[0] and st["operations"]["split"][0] > 300
    rep = Dm.manifold_report(fo, vo.shape[0])
    assert rep["duplicates"] == 0 and rep["degenerate"] == 0 and rep["euler"] == 1
    before, after = Rm.measures(v, f), Rm.measures(vo, fo)
    record_parity("mesh_remesh_loop[grid]", {"faces_before": int(f.shape[0]), "faces_after": int(fo.shape[0]), "operations": st["operations"],
                                             "rounds": st["rounds"], "before": before, "after": after, "distance": st["distance"]["hausdorff"]})


def test_the_capacity_runs_out_and_the_run_goes_on(monkeypatch):
    name = "ico3"
    v, f, c = Rm.decimated(name)
    monkeypatch.setattr(MR, "MIN_SPARE", 48)
    monkeypatch.setattr(MR, "SPARE_SHARE", 0.0)                                              # 48 spare rows: the first split pass needs 70
    vo, fo, co, st = MR.remesh_mesh(v, f, c, iterations=3)
    vo, fo = vo.cpu().numpy(), fo.cpu().numpy().astype(np.int64)
    assert st["reallocations"] == 1 and st["operations"]["split"][0] >= 70
    assert Dm.manifold_report(fo, vo.shape[0]) == {**CLOSED, "used_vertices": vo.shape[0]}
    before, mine, want = Rm.measures(v, f), Rm.measures(vo, fo), Rm.measures(*Rm.loop_run(name)[:2])
    record_parity("mesh_remesh_loop[ico3, one reallocation]", {"faces_after": int(fo.shape[0]), "operations": st["operations"], "rounds": st["rounds"],
                                                               "after": mine})
    for k, sign in Rm.MEASURES.items():
        assert (mine[k] - before[k]) * sign >= 0.5 * (want[k] - before[k]) * sign, k


def test_rounds_without_an_end_are_an_error():
    v, f, c = Rm.decimated("ico3")
    with pytest.raises(RuntimeError, match="split pass did not end within 2 rounds"):
        MR.remesh_mesh(v, f, c, iterations=1, max_rounds=2)


# ---- 4. the script, and nothing to do ---------------------------------------------------------------------------------------------------------
def test_script_output_feeds_the_other_mesh_scripts(tmp_path):
    v, f, c = Rm.decimated("net")
    ply, out = str(tmp_path / "mesh.ply"), str(tmp_path / "even.ply")
    G.save_mesh_ply(ply, v, f, c)
    rv0, rf0, rc0 = G.read_mesh_ply(ply)
    _entry("remesh_mesh").main(["--mesh", ply, "-o", out, "--iterations", "3"])
    stats = json.load(open(tmp_path / "even.json"))
    rv, rf, rc = G.read_mesh_ply(out)
    assert stats["faces_after"] == rf.shape[0] and stats["vertices_after"] == rv.shape[0] and rc.shape == rv.shape
    assert Dm.manifold_report(rf, rv.shape[0]) == {**CLOSED, "used_vertices": rv.shape[0]}
    direct = MR.remesh_mesh(rv0, rf0, rc0.astype(np.float32) / 255.0, iterations=3)          # (the PLY holds the colours as bytes)
    assert np.array_equal(direct[0].cpu().numpy(), rv) and np.array_equal(direct[1].cpu().numpy(), rf)
    orbit = str(tmp_path / "orbit")
    _entry("render_mesh").main(["--mesh", out, "-o", orbit, "--render_orbit", "1", "--reso", "32", "-w"])
    assert sorted(os.listdir(orbit)) == ["000.png", "orbit.npy"]
    small = str(tmp_path / "small.ply")
    _entry("decimate_mesh").main(["--mesh", out, "-o", small, "--target_faces", "300"])
    ds = json.load(open(tmp_path / "small.json"))
    assert ds["faces_before"] == rf.shape[0] and ds["faces_after"] in (300, 299) and ds["boundary_vertices_after"] == 0


def test_nothing_to_do_is_answered_without_a_launch():
    v, f, c = Dm.scene("ico2")
    none = torch.zeros(0, 3, dtype=torch.int64)
    for vv, ff, cc in ((v, none, c), (v[:0], none, c[:0])):
        ov, of, oc, st = MR.remesh_mesh(vv, ff, cc)
        assert ov.device.type == "cuda" and torch.equal(ov.cpu(), vv) and of.shape == (0, 3) and torch.equal(oc.cpu(), cc) and st["faces_after"] == 0
    ov, of, oc, st = MR.remesh_mesh(v, f, None, iterations=0)
    assert torch.equal(ov.cpu(), v) and torch.equal(of.cpu().long(), f) and oc is None and st["operations"] == {"split": [], "collapse": [], "flip": []}
