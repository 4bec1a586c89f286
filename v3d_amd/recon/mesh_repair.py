"""Repair what check_mesh reports, on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshrepair.hip, include/v3d_recon.h "Mesh repair"), and
keep every triangle there is no reason to touch: weld the vertices that coincide, drop the faces that are none, give every orientable patch
one winding (outwards where the patch is closed), cut out the faces that pass through each other or hang on a non-manifold, pinched or
wrongly wound vertex, and fan the open loops shut.

    remap = weld_remap(verts)                                  # [V] int32: the smallest index at the same position
    bits = drop_flags(verts, faces)                            # [F] int32: 1 absent, 2 repeated index, 4 no area, 8 duplicate
    faces, info = orient_faces(verts, faces)                   # info: rounds, non_orientable, flipped_patches
    verts, faces, colors, info = repair_mesh(verts, faces, colors)

The checks inside the loop are those of mesh_check.py (the self-pair walk on the BVH, the census on the corner lists); the sorts and scans are
v3d_gs_radix_sort_pairs and v3d_gs_scan.  No atomics anywhere: two calls with the same arguments return bit-equal results.  Everything runs
under no_grad.  There is no fallback: without the libraries this raises."""
from __future__ import annotations

import time

import numpy as np
import torch

from ..ops import get_ops
from . import mesh_check as MK
from . import mesh_clean as MC
from .geometry import _check, _stream, load_library
from .mesh_bake import build_bvh
from .mesh_query import _int_arg

INT32_MAX = 2 ** 31 - 1
DOUBLING_ROUNDS = 32
ROUND_GROUP = 8                    # orient rounds between two reads of the change flags
ABSENT, REPEATED, NO_AREA, DUPLICATE = 1, 2, 4, 8             # the bits of v3d_recon_repair_drop_flags
HISTORY_KEYS = ("faces", "pairs", "bad_vertices", "open_edges", "faces_cut", "loops_filled", "loops_left", "vertices_added", "faces_filled",
                "faces_dropped", "faces_after")


def _i32(n, dev):
    return torch.empty(n, dtype=torch.int32, device=dev)


def _call(name, *args):
    lib = load_library()
    _check(lib, getattr(lib, name)(*args, _stream()), name)


class _Clock:
    """seconds per pass into `timings` (each lap ended by a synchronize), or nothing at all"""

    def __init__(self, timings):
        self.t, self.timings = time.perf_counter(), timings

    def lap(self, name):
        if self.timings is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.timings[name] = self.timings.get(name, 0.0) + now - self.t
            self.t = now


# ---- the passes, on validated device tensors (V >= 1, F >= 1) -------------------------------------------------------------------------------
def _weld_remap(v):
    V, dev, ops = v.shape[0], v.device, get_ops()
    kz, kxy = torch.empty(V, dtype=torch.int64, device=dev), torch.empty(V, dtype=torch.int64, device=dev)
    vals = _i32(V, dev)
    _call("v3d_recon_repair_weld_keys", v.data_ptr(), V, kz.data_ptr(), kxy.data_ptr(), vals.data_ptr())
    _, by_z = ops.gs_radix_sort_pairs(kz, vals, 32)
    _, order = ops.gs_radix_sort_pairs(kxy[by_z.long()].contiguous(), by_z, 64)
    heads = _i32(V, dev)
    _call("v3d_recon_repair_weld_heads", v.data_ptr(), V, order.data_ptr(), heads.data_ptr())
    offsets = ops.gs_scan(heads)
    first, remap = _i32(V, dev), _i32(V, dev)
    _call("v3d_recon_repair_weld_first", order.data_ptr(), heads.data_ptr(), offsets.data_ptr(), V, first.data_ptr())
    _call("v3d_recon_repair_weld_remap", order.data_ptr(), offsets.data_ptr(), first.data_ptr(), V, remap.data_ptr())
    return remap


def _remap_faces(f, V, remap):
    out = torch.empty_like(f)
    _call("v3d_recon_repair_remap_faces", f.data_ptr(), f.shape[0], V, remap.data_ptr(), out.data_ptr())
    return out


def _drop_flags(v, f):
    ranges, corners = MC._corner_lists(f, v.shape[0])
    bits = _i32(f.shape[0], f.device)
    _call("v3d_recon_repair_drop_flags", v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(), bits.data_ptr())
    return bits


def _keep_faces(f, V, keep):
    """the faces with keep != 0, in their order, through the scan and v3d_recon_mesh_compact_faces (every vertex stays)"""
    offs = get_ops().gs_scan(keep)
    n = int(offs[-1].item())
    if n == 0:
        return f[:0].contiguous()
    if n == f.shape[0]:
        return f
    every = torch.ones(V, dtype=torch.int32, device=f.device)
    same_index = torch.arange(V + 1, dtype=torch.int32, device=f.device)
    out = torch.empty(n, 3, dtype=torch.int32, device=f.device)
    _call("v3d_recon_mesh_compact_faces", f.data_ptr(), f.shape[0], V, keep.data_ptr(), offs.data_ptr(), every.data_ptr(), same_index.data_ptr(), n, V,
          out.data_ptr())
    return out


def _drop(v, f):
    return _keep_faces(f, v.shape[0], (_drop_flags(v, f) == 0).to(torch.int32))


def _orient_labels(f, V, ranges, corners, same, opposite):
    """(labels [F] int32 at the fixed point, rounds up to and including the first that changed nothing), in groups as mesh_clean._labels"""
    F = f.shape[0]
    cur = 2 * torch.arange(F, dtype=torch.int32, device=f.device)
    nxt = torch.empty_like(cur)
    flags = _i32(ROUND_GROUP, f.device)
    done, limit = 0, F + 8
    while done < limit:
        group = min(ROUND_GROUP, limit - done)
        flags.zero_()
        for j in range(group):
            _call("v3d_recon_repair_orient_round", f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(),
                  cur.data_ptr(), nxt.data_ptr(), flags.data_ptr() + 4 * j)
            cur, nxt = nxt, cur
        changed = flags.cpu().tolist()[:group]
        if 0 in changed:
            return cur, done + changed.index(0) + 1
        done += group
    raise RuntimeError(f"orient_faces: no fixed point after {limit} rounds on {F} faces: the corner lists are broken")


def _orient_apply(f, labels, nonorient, patch_flip=None):
    out = torch.empty_like(f)
    _call("v3d_recon_repair_orient_apply", f.data_ptr(), f.shape[0], labels.data_ptr(), nonorient.data_ptr(),
          patch_flip.data_ptr() if patch_flip is not None else None, out.data_ptr())
    return out


def patch_flips(verts, faces, labels, same, opposite, nonorient):
    """[F] int32 by root: 1 for every orientable patch without an open edge whose signed volume, summed in float64 in face order, is negative
    (host arrays; not hot)"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f, lab = np.asarray(faces).reshape(-1, 3), np.asarray(labels)
    roots = (lab >> 1).tolist()
    is_open = ((np.asarray(same) + np.asarray(opposite)).reshape(-1, 3) == 1).any(1)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    t = ((a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]))
         + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])).tolist()
    vol, open_roots = {}, {r for r, o in zip(roots, is_open.tolist()) if o}
    for r, x in zip(roots, t):
        vol[r] = vol.get(r, 0.0) + x
    flip = np.zeros(f.shape[0], dtype=np.int32)
    marks = np.asarray(nonorient)
    for r, x in vol.items():
        if x < 0 and r not in open_roots and not marks[r]:
            flip[r] = 1
    return flip


def _orient(v, f, clock=None):
    V, F = v.shape[0], f.shape[0]
    ranges, corners = MC._corner_lists(f, V)
    same, opposite, _ = MK._census(f, V)
    labels, rounds = _orient_labels(f, V, ranges, corners, same, opposite)
    nonorient = torch.zeros(F, dtype=torch.int32, device=f.device)
    _call("v3d_recon_repair_orient_conflicts", f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(),
          labels.data_ptr(), nonorient.data_ptr())
    out = _orient_apply(f, labels, nonorient)
    if clock is not None:
        clock.lap("orient")
    flip = patch_flips(v.cpu().numpy(), out.cpu().numpy(), labels.cpu().numpy(), same.cpu().numpy(), opposite.cpu().numpy(), nonorient.cpu().numpy())
    if flip.any():
        out = _orient_apply(out, labels & ~1, nonorient, torch.from_numpy(flip).to(f.device))
    if clock is not None:
        clock.lap("orient_volume")
    return out, {"rounds": rounds, "non_orientable": int(nonorient.sum()), "flipped_patches": int(flip.sum())}


def _vertex_open(f, V, ranges, corners, same, opposite, flags):
    bad, nxt = _i32(V, f.device), _i32(V, f.device)
    _call("v3d_recon_repair_vertex_open", f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(),
          flags.data_ptr(), bad.data_ptr(), nxt.data_ptr())
    return bad, nxt


def _trouble(f, V, per_face, bad):
    out = _i32(f.shape[0], f.device)
    _call("v3d_recon_repair_trouble", f.data_ptr(), f.shape[0], V, per_face.data_ptr(), bad.data_ptr(), out.data_ptr())
    return out


def _grow(f, V, ranges, corners, marks):
    out = torch.empty_like(marks)
    _call("v3d_recon_repair_grow", f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(), V, marks.data_ptr(), out.data_ptr())
    return out


def _loop_labels(bad, nxt):
    V = bad.shape[0]
    lab, jump = torch.arange(V, dtype=torch.int32, device=bad.device), torch.where(bad != 0, torch.full_like(nxt, -1), nxt).contiguous()
    lab2, jump2 = torch.empty_like(lab), torch.empty_like(jump)
    for _ in range(DOUBLING_ROUNDS):
        _call("v3d_recon_repair_loop_round", V, lab.data_ptr(), jump.data_ptr(), lab2.data_ptr(), jump2.data_ptr())
        lab, lab2, jump, jump2 = lab2, lab, jump2, jump
    return lab, jump


def _loop_flags(bad, nxt, lab, jump, cap: int):
    """(state [V], length [V], loop_ranges [V, 2], members [V])"""
    V, dev = bad.shape[0], bad.device
    live = (jump >= 0) & (jump < V)
    keys = torch.where(live, lab, torch.full_like(lab, V)).to(torch.int64).contiguous()
    keys_s, members = get_ops().gs_radix_sort_pairs(keys, torch.arange(V, dtype=torch.int32, device=dev), max(1, V.bit_length()))
    ranges = torch.empty(V, 2, dtype=torch.int32, device=dev)
    _call("v3d_recon_mesh_vertex_ranges", keys_s.data_ptr(), V, V, ranges.data_ptr())
    state, length = _i32(V, dev), _i32(V, dev)
    _call("v3d_recon_repair_loop_flags", V, nxt.data_ptr(), bad.data_ptr(), lab.data_ptr(), jump.data_ptr(), ranges.data_ptr(), members.data_ptr(), cap,
          state.data_ptr(), length.data_ptr())
    return state, length, ranges, members


def _fill_emit(v, c, nxt, ranges, members, state, length):
    """(new faces [n, 3] int32, new verts [m, 3], new colours [m, 3] or None) of the fillable loops (at least one)"""
    V, dev, ops = v.shape[0], v.device, get_ops()
    fillable = state == 1
    face_off = ops.gs_scan(torch.where(fillable, torch.where(length == 3, torch.ones_like(length), length), torch.zeros_like(length)).contiguous())
    vert_off = ops.gs_scan((fillable & (length > 3)).to(torch.int32))
    nf, nv = int(face_off[-1].item()), int(vert_off[-1].item())
    if V + nv > INT32_MAX:
        raise ValueError(f"repair_mesh: {V} + {nv} vertices exceed {INT32_MAX}")
    new_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    new_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    new_c = torch.empty(nv, 3, dtype=torch.float32, device=dev) if c is not None else None
    _call("v3d_recon_repair_fill_emit", v.data_ptr(), c.data_ptr() if c is not None else None, V, nxt.data_ptr(), ranges.data_ptr(), members.data_ptr(),
          state.data_ptr(), length.data_ptr(), face_off.data_ptr(), vert_off.data_ptr(), nf, nv, new_f.data_ptr(), new_v.data_ptr() if nv else None,
          new_c.data_ptr() if c is not None and nv else None)
    return new_f, new_v, new_c


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def _mesh_args(verts, faces, colors, device, who: str):
    v = MC._rows_arg(verts, "cpu", who, "verts")
    if v.shape[0] == 0 or v.shape[0] > INT32_MAX:
        raise ValueError(f"{who}: {v.shape[0]} vertices")
    if not bool(torch.isfinite(v).all()):
        raise ValueError(f"{who}: a vertex is not finite")
    f, V = MK._census_faces(faces, v.shape[0], "cpu", who)
    c = None
    if colors is not None:
        c = MC._rows_arg(colors, "cpu", who, "colors")
        if c.shape != v.shape:
            raise ValueError(f"{who}: {v.shape[0]} vertices, {c.shape[0]} colours")
    return v.to(device), f.to(device), (c.to(device) if c is not None else None)


def _flag(value, who: str, name: str) -> bool:
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{who}: {name} {value!r} must be True or False")
    return bool(value)


# ---- the public functions -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def weld_remap(verts, device="cuda") -> torch.Tensor:
    """remap [V] int32: the smallest index among the vertices whose three float32 coordinates equal v's by value (-0.0 equals +0.0)"""
    v, _, _ = _mesh_args(verts, torch.zeros(1, 3, dtype=torch.int32), None, device, "weld_remap")
    return _weld_remap(v)


@torch.no_grad()
def drop_flags(verts, faces, device="cuda") -> torch.Tensor:
    """bits [F] int32: ABSENT alone, or the OR of REPEATED, NO_AREA and DUPLICATE (a face of a lower index holds the same three vertices)"""
    v, f, _ = _mesh_args(verts, faces, None, device, "drop_flags")
    return _drop_flags(v, f)


@torch.no_grad()
def orient_faces(verts, faces, device="cuda"):
    """(faces [F, 3] int32, {"rounds", "non_orientable", "flipped_patches"}): every orientable patch wound like its smallest face, and a
    closed patch of negative volume flipped whole;  a patch that cannot be wound one way is left as it is and counted."""
    v, f, _ = _mesh_args(verts, faces, None, device, "orient_faces")
    return _orient(v, f)


@torch.no_grad()
def repair_mesh(verts, faces, colors=None, *, grow: int = 1, max_rounds: int = 8, max_hole_edges=None, orient: bool = True, weld: bool = True,
                device="cuda", timings: dict = None):
    """(verts [V', 3] float32, faces [F', 3] int32, colors [V', 3] float32 or None, info).  Weld, drop and orient run once; then up to
    max_rounds rounds of check (pairs and census), cut (the faces in an intersecting pair or on a bad vertex, grown `grow` times over shared
    vertices), fill (every open loop of 3 .. max_hole_edges edges through good vertices: one face, or a fan about the loop's centre), drop,
    and orient where a round left an edge wound wrongly.  The loop stops at the first round with nothing to cut and nothing to fill
    ("clean"), when a round would leave no face ("empty": the state before that round is returned), when a round without a cut leaves
    the faces as they were ("stalled": every new face was a duplicate) or after max_rounds.  At the end the vertices that no face uses are
    removed, in order.  A mesh with nothing to repair comes back bit-equal with an empty history.
    info: "before", "after" (check_mesh), "history" (one dict of HISTORY_KEYS per round that changed the mesh: faces(r + 1) = faces(r) -
    faces_cut + faces_filled - faces_dropped), "stopped", "orient" (of the first pass), "loops_left" (open loops of the last round that
    were not fillable).  timings, when given, receives the seconds per pass summed over the rounds."""
    who = "repair_mesh"
    n_grow = _int_arg(grow, 0, 64, who, "grow")
    n_rounds = _int_arg(max_rounds, 0, 1024, who, "max_rounds")
    cap = INT32_MAX if max_hole_edges is None else _int_arg(max_hole_edges, 3, INT32_MAX, who, "max_hole_edges")
    do_orient, do_weld = _flag(orient, who, "orient"), _flag(weld, who, "weld")
    v, f, c = _mesh_args(verts, faces, colors, device, who)
    f_in = f
    before = MK.check_mesh(v, f, device)
    clock = _Clock(timings)
    if do_weld:
        f = _remap_faces(f, v.shape[0], _weld_remap(v))
        clock.lap("weld")
    f = _drop(v, f)
    clock.lap("drop")
    if f.shape[0] == 0:
        raise ValueError(f"{who}: nothing is left of the mesh: every face is absent, repeats an index, has no area or is a duplicate")
    info = {"rounds": 0, "non_orientable": 0, "flipped_patches": 0}
    if do_orient:
        f, info = _orient(v, f, clock)
    history, stopped, left = [], "max_rounds", 0
    for _ in range(n_rounds):
        V = v.shape[0]
        per_face, n_up = MK._self_count(build_bvh(v, f, device))
        pairs = int(n_up.sum(dtype=torch.int64))
        ranges, corners = MC._corner_lists(f, V)
        same, opposite, flags = MK._census(f, V)
        clock.lap("check")
        bad, nxt = _vertex_open(f, V, ranges, corners, same, opposite, flags)
        marks = _trouble(f, V, per_face, bad)
        cut, g = 0, f
        if bool(marks.any()):
            for _ in range(n_grow):
                marks = _grow(f, V, ranges, corners, marks)
            g = _keep_faces(f, V, (marks == 0).to(torch.int32))
            cut = f.shape[0] - g.shape[0]
        clock.lap("cut")
        if g.shape[0] == 0:
            stopped = "empty"
            break
        bad2, nxt2 = bad, nxt
        if cut:
            r2, c2 = MC._corner_lists(g, V)
            s2, o2, fl2 = MK._census(g, V)
            bad2, nxt2 = _vertex_open(g, V, r2, c2, s2, o2, fl2)
        lab, jump = _loop_labels(bad2, nxt2)
        state, length, loop_ranges, members = _loop_flags(bad2, nxt2, lab, jump, cap)
        filled, left = int((state == 1).sum()), int((state == 2).sum())
        if cut == 0 and filled == 0:
            clock.lap("fill")
            stopped = "clean"
            break
        v2, c_2, h, added, n_new = v, c, g, 0, 0
        if filled:
            new_f, new_v, new_c = _fill_emit(v, c, nxt2, loop_ranges, members, state, length)
            added, n_new = new_v.shape[0], new_f.shape[0]
            h = torch.cat([g, new_f]).contiguous()
            if added:
                v2 = torch.cat([v, new_v]).contiguous()
                c_2 = torch.cat([c, new_c]).contiguous() if c is not None else None
        clock.lap("fill")
        n_before_drop = h.shape[0]
        h = _drop(v2, h)
        clock.lap("drop")
        if h.shape[0] == 0:
            stopped = "empty"
            break
        if cut == 0 and h.shape == f.shape and torch.equal(h, f):
            stopped = "stalled"
            break
        if do_orient and bool((MK._census(h, v2.shape[0])[2] & MK.WINDING).any()):
            h, _ = _orient(v2, h, clock)
        history.append(dict(zip(HISTORY_KEYS, (f.shape[0], pairs, int(bad.sum()), int(((same == 1) & (opposite == 0)).sum()), cut, filled, left, added,
                                               n_new, n_before_drop - h.shape[0], h.shape[0]))))
        v, c, f = v2, c_2, h
    untouched = stopped == "clean" and not history and f.shape == f_in.shape and torch.equal(f, f_in)
    if not untouched:
        V = v.shape[0]
        ranges, corners = MC._corner_lists(f, V)
        v, f, c, _ = MC._compact(v, f, c, ranges, corners, torch.zeros(V, dtype=torch.int32, device=f.device), [0])
    after = MK.check_mesh(v, f, device)
    return v, f, c, {"before": before, "after": after, "history": history, "stopped": stopped, "orient": info, "loops_left": left}
