"""Decimate the extracted mesh on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshdecim.hip, include/v3d_recon.h "Mesh decimation"):
quadric-error half-edge collapse in parallel rounds, down to a target number of faces - what the reference's fit_mesh does first
(decimate_target = 5e4) before it unwraps and textures.

    verts, faces, colors, stats = decimate_mesh(verts, faces, colors, 50000)

    Q = vertex_quadrics(verts, faces)                                  # the steps of one round, for the tests
    keys, targets = propose(verts, faces, Q)
    accept, flags = select(faces, V, keys)
    accept = cut(keys, accept, live_faces, target_faces)
    faces, live, Q = apply(faces, V, accept, targets, Q)

A collapse v -> u moves v onto u; u keeps its position and colour, so the output's vertices are a subset of the input's, in their order,
bit-equal.  Vertices on open edges and non-manifold vertices are never removed.  The vertex -> corner lists are those of mesh_clean.py,
rebuilt every round from the live faces; every kernel has one owner per output and there are no atomics: two calls with the same arguments
return bit-equal results.  Everything runs under no_grad.  There is no fallback: without the libraries this raises.  V = 0, F = 0 and
target_faces >= F are answered without a launch."""
from __future__ import annotations

import math
import struct

import torch

from ..ops import get_ops
from .geometry import _check, _stream, load_library
from .mesh_clean import INT32_MAX, _boundary, _corner_lists, _count_arg, _faces_arg, _mesh_arg

DEFAULT_MAX_VALENCE = 24           # faces around a vertex: one above it proposes nothing, and no collapse may lift its target above it
MAX_VALENCE_LIMIT = 1024           # V3D_RECON_MESH_MAX_VALENCE
ROUND_GROUP = 4                    # rounds between two reads of the live-face counts and the flags
NO_KEY = -1                        # all ones, as the int64 that holds the uint64 key


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def _valence_arg(value, who: str) -> int:
    value = _count_arg(value, who, "max_valence")
    if not 3 <= value <= MAX_VALENCE_LIMIT:
        raise ValueError(f"{who}: max_valence {value} outside 3 .. {MAX_VALENCE_LIMIT}")
    return value


def _error_arg(value, who: str) -> float:
    """max_error as the float the kernel compares fp32 costs against: +inf for None"""
    if value is None:
        return math.inf
    value = float(value)
    if not value >= 0:
        raise ValueError(f"{who}: max_error {value} must be a number that is not negative")
    return value


def _keys_arg(keys, V: int, device, who: str, name: str = "keys") -> torch.Tensor:
    k = keys.detach() if torch.is_tensor(keys) else torch.as_tensor(keys)
    if k.dtype != torch.int64 or tuple(k.shape) != (V,):
        raise ValueError(f"{who}: {name} must be int64 [{V}], got {k.dtype} {tuple(k.shape)}")
    return k.to(device).contiguous()


def _ints_arg(a, V: int, device, who: str, name: str) -> torch.Tensor:
    t = a.detach() if torch.is_tensor(a) else torch.as_tensor(a)
    if t.is_floating_point() or t.is_complex() or tuple(t.shape) != (V,):
        raise ValueError(f"{who}: {name} must be integers [{V}], got {t.dtype} {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _quadrics_arg(q, V: int, device, who: str) -> torch.Tensor:
    t = q.detach() if torch.is_tensor(q) else torch.as_tensor(q)
    if t.dtype != torch.float64 or tuple(t.shape) != (V, 10):
        raise ValueError(f"{who}: quadrics must be float64 [{V}, 10], got {t.dtype} {tuple(t.shape)}")
    return t.to(device).contiguous()


def cost_of_key(keys: torch.Tensor) -> torch.Tensor:
    """The fp32 costs held in the high halves of `keys` (int64 [n]); nan for a key of all ones"""
    return (keys >> 32).to(torch.int32).view(torch.float32)


def _bits_to_float(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]


# ---- the kernels, on validated device tensors (V >= 1, F >= 1) ------------------------------------------------------------------------------
def _live_lists(f: torch.Tensor, V: int):
    """The corner lists of the live faces: the dead ones hold V, and with V + 1 vertices their corners gather on the extra one"""
    ranges, corners = _corner_lists(f, V + 1)
    return ranges, corners


def _quadrics(v, f, ranges, corners):
    lib = load_library()
    Q = torch.empty(v.shape[0], 10, dtype=torch.float64, device=v.device)
    _check(lib, lib.v3d_recon_mesh_vertex_quadrics(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(),
                                                   Q.data_ptr(), _stream()), "v3d_recon_mesh_vertex_quadrics")
    return Q


def _propose(v, f, ranges, corners, Q, max_valence: int):
    lib = load_library()
    V = v.shape[0]
    keys = torch.empty(V, dtype=torch.int64, device=v.device)
    targets = torch.empty(V, dtype=torch.int32, device=v.device)
    _check(lib, lib.v3d_recon_mesh_decim_propose(v.data_ptr(), V, f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(), Q.data_ptr(),
                                                 max_valence, keys.data_ptr(), targets.data_ptr(), _stream()), "v3d_recon_mesh_decim_propose")
    return keys, targets


def _select(f, V: int, ranges, corners, keys, max_error: float, flags: torch.Tensor):
    """(accept [V] int32, sel_keys [V], sel_vals [V]); flags: two cleared int32 words on the device"""
    lib = load_library()
    min1, min2 = torch.empty_like(keys), torch.empty_like(keys)
    for src, dst in ((keys, min1), (min1, min2)):
        _check(lib, lib.v3d_recon_mesh_decim_min_round(f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(), V, src.data_ptr(),
                                                       dst.data_ptr(), _stream()), "v3d_recon_mesh_decim_min_round")
    accept = torch.empty(V, dtype=torch.int32, device=f.device)
    sel_keys, sel_vals = torch.empty_like(keys), torch.empty(V, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_decim_accept(keys.data_ptr(), min2.data_ptr(), V, max_error, accept.data_ptr(), sel_keys.data_ptr(),
                                                sel_vals.data_ptr(), flags.data_ptr(), _stream()), "v3d_recon_mesh_decim_accept")
    return accept, sel_keys, sel_vals


def _cut(accept, sel_keys, sel_vals, live: torch.Tensor, target: int):
    """Clears, in place, the accepted vertices beyond what `target` allows; live: the number of live faces, one int32 on the device"""
    lib, ops = load_library(), get_ops()
    ks, vs = ops.gs_radix_sort_pairs(sel_keys, sel_vals, 64)
    _check(lib, lib.v3d_recon_mesh_decim_cut(ks.data_ptr(), vs.data_ptr(), accept.shape[0], live.data_ptr(), target, accept.data_ptr(), _stream()),
           "v3d_recon_mesh_decim_cut")
    return accept


def _apply(f, V: int, accept, targets, Q, removed):
    """(faces_out, live [F]); Q and removed are updated in place"""
    lib = load_library()
    out = torch.empty_like(f)
    live = torch.empty(f.shape[0], dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_decim_apply(f.data_ptr(), f.shape[0], V, accept.data_ptr(), targets.data_ptr(), out.data_ptr(), live.data_ptr(),
                                               Q.data_ptr(), removed.data_ptr(), _stream()), "v3d_recon_mesh_decim_apply")
    return out, live


# ---- the steps of a round, public ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def vertex_quadrics(verts, faces, device="cuda") -> torch.Tensor:
    """Q [V, 10] float64: per vertex the sum, in list order, of the area-weighted plane quadrics of its faces (aa ab ac ad bb bc bd cc cd dd)"""
    v, f, _ = _mesh_arg(verts, faces, None, device, "vertex_quadrics")
    if v.shape[0] == 0 or f.shape[0] == 0:
        return torch.zeros(v.shape[0], 10, dtype=torch.float64, device=device)
    return _quadrics(v, f, *_live_lists(f, v.shape[0]))


@torch.no_grad()
def propose(verts, faces, quadrics, max_valence: int = DEFAULT_MAX_VALENCE, device="cuda"):
    """(keys [V] int64, targets [V] int32): every removable vertex's cheapest valid collapse, key = fp32 bits of the cost << 32 | v; a key of
    all ones (-1) and target -1 where there is none (v3d_recon_mesh_decim_propose has the rules)"""
    max_valence = _valence_arg(max_valence, "propose")
    v, f, _ = _mesh_arg(verts, faces, None, device, "propose")
    V = v.shape[0]
    Q = _quadrics_arg(quadrics, V, device, "propose")
    if V == 0 or f.shape[0] == 0:
        return torch.full((V,), NO_KEY, dtype=torch.int64, device=device), torch.full((V,), -1, dtype=torch.int32, device=device)
    return _propose(v, f, *_live_lists(f, V), Q, max_valence)


@torch.no_grad()
def select(faces, num_verts: int, keys, max_error=None, device="cuda"):
    """(accept [V] int32, flags): accept = 1 where the vertex's key is not all ones, is the smallest within graph distance 2 and costs at most
    max_error; flags = (a local minimum exists, one was accepted)"""
    max_error = _error_arg(max_error, "select")
    f = _faces_arg(faces, num_verts, device, "select")
    V = int(num_verts)
    k = _keys_arg(keys, V, device, "select")
    if V == 0 or f.shape[0] == 0:
        return torch.zeros(V, dtype=torch.int32, device=device), (False, False)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    accept, _, _ = _select(f, V, *_live_lists(f, V), k, max_error, flags)
    return accept, tuple(bool(x) for x in flags.tolist())


@torch.no_grad()
def cut(keys, accept, live_faces: int, target_faces: int, device="cuda") -> torch.Tensor:
    """accept [V] int32 with only the ceil((live_faces - target_faces) / 2) accepted vertices of the smallest keys left (every collapse
    removes two faces); none when live_faces <= target_faces"""
    live_faces, target_faces = _count_arg(live_faces, "cut", "live_faces"), _count_arg(target_faces, "cut", "target_faces")
    if max(live_faces, target_faces) > INT32_MAX:
        raise ValueError(f"cut: live_faces {live_faces} and target_faces {target_faces} must not exceed {INT32_MAX}")
    a = accept.detach() if torch.is_tensor(accept) else torch.as_tensor(accept)
    V = a.shape[0] if a.dim() == 1 else -1
    a = _ints_arg(a, V, device, "cut", "accept").clone()
    k = _keys_arg(keys, V, device, "cut")
    if V == 0:
        return a
    on = a != 0
    sel_keys = torch.where(on, k, torch.full_like(k, NO_KEY))
    sel_vals = torch.arange(V, dtype=torch.int32, device=device)
    return _cut(a, sel_keys, sel_vals, torch.tensor([live_faces], dtype=torch.int32, device=device), target_faces)


@torch.no_grad()
def apply(faces, num_verts: int, accept, targets, quadrics, device="cuda"):
    """(faces [F, 3] int32, live [F] int32, Q [V, 10]) after the accepted collapses: a face on a collapsed edge is dead (live 0; its row
    holds V V V), a face with an accepted vertex alone names its target instead; Q[target] += Q[v].  The accepted set must be one that
    `select` made (no face with two accepted vertices, distinct targets)."""
    f = _faces_arg(faces, num_verts, device, "apply")
    V = int(num_verts)
    a, t = _ints_arg(accept, V, device, "apply", "accept"), _ints_arg(targets, V, device, "apply", "targets")
    Q = _quadrics_arg(quadrics, V, device, "apply").clone()
    if V == 0 or f.shape[0] == 0:
        return f, torch.ones(f.shape[0], dtype=torch.int32, device=device), Q
    out, live = _apply(f, V, a, t, Q, torch.zeros(V, dtype=torch.int32, device=device))
    return out, live, Q


# ---- the whole ------------------------------------------------------------------------------------------------------------------------------------
def _stats(F: int, target: int, boundary: int) -> dict:
    return {"faces_before": F, "faces_after": F, "target_faces": target, "rounds": 0, "accepted": [], "reached": F <= target,
            "stopped": "target" if F <= target else None, "max_cost": 0.0, "boundary_vertices_before": boundary, "boundary_vertices_after": boundary}


@torch.no_grad()
def decimate_mesh(verts, faces, colors, target_faces: int, *, max_error=None, max_valence: int = DEFAULT_MAX_VALENCE, max_rounds=None,
                  device="cuda"):
    """(verts, faces, colors, stats) with at most target_faces faces where the mesh allows it: rounds of quadric-error half-edge collapses
    (module docstring), the last one cut so that the result has target_faces faces or one less.  colors may be None.

    max_error: stop as soon as the cheapest proposal costs more (the cost is the sum of squared distances, each weighted by its face's area,
    of the target's position to the planes gathered on the two vertices; None: no limit).  max_valence: a vertex with more faces is never
    removed and no collapse may leave its target with more (default 24: surface nets give 4 - 10, and a cap keeps the lists every thread
    walks short).  max_rounds: RuntimeError when that many rounds did not end the run (None: F / 2 + 8, which no run can need).

    What stays keeps its order and its bits; the vertices that no collapse removed stay, those that no face used before included.
    stats (json.dumps takes it): "faces_before" / "faces_after", "vertices_before" / "vertices_after", "target_faces", "rounds", "accepted"
    (collapses per round), "reached" (faces_after <= target_faces), "stopped" ("target", "no valid collapse" or "max_error"), "max_cost" (the
    largest accepted cost), "boundary_vertices_before" / "boundary_vertices_after"."""
    who = "decimate_mesh"
    target = _count_arg(target_faces, who, "target_faces")
    max_error = _error_arg(max_error, who)
    max_valence = _valence_arg(max_valence, who)
    if max_rounds is not None:
        max_rounds = _count_arg(max_rounds, who, "max_rounds")
    v, f, c = _mesh_arg(verts, faces, colors, device, who)
    V, F = v.shape[0], f.shape[0]
    if V == 0 or F == 0 or target >= F:
        stats = _stats(F, target, None if V and F else 0)          # (nothing to do: no launch, so the open edges of a mesh with faces are not counted)
        stats.update(vertices_before=V, vertices_after=V)
        return v, f, c, stats
    lib, ops = load_library(), get_ops()
    target = min(target, INT32_MAX)
    ranges, corners = _live_lists(f, V)
    stats = _stats(F, target, int(_boundary(f, V, ranges, corners).sum()))
    stats.update(vertices_before=V)
    Q = _quadrics(v, f, ranges, corners)
    removed = torch.zeros(V, dtype=torch.int32, device=f.device)
    live_count = torch.tensor([F], dtype=torch.int32, device=f.device)
    live = torch.ones(F, dtype=torch.int32, device=f.device)
    limit = max_rounds if max_rounds is not None else F // 2 + 8
    cur, faces_live, stopped = f, F, None
    counts = torch.empty(ROUND_GROUP, dtype=torch.int32, device=f.device)
    flags = torch.empty(ROUND_GROUP, 2, dtype=torch.int32, device=f.device)
    costs = torch.empty(ROUND_GROUP, dtype=torch.int64, device=f.device)
    while stopped is None:
        if stats["rounds"] >= limit:
            raise RuntimeError(f"{who}: {faces_live} faces left after {limit} rounds, target {target}")
        group = min(ROUND_GROUP, limit - stats["rounds"])
        flags.zero_()
        for j in range(group):
            if j:
                ranges, corners = _live_lists(cur, V)
            keys, targets = _propose(v, cur, ranges, corners, Q, max_valence)
            accept, sel_keys, sel_vals = _select(cur, V, ranges, corners, keys, max_error, flags[j])
            _cut(accept, sel_keys, sel_vals, live_count, target)
            costs[j] = torch.where(accept != 0, keys >> 32, torch.zeros_like(keys)).max()
            cur, live = _apply(cur, V, accept, targets, Q, removed)
            live_off = ops.gs_scan(live)
            live_count = live_off[F:]
            counts[j] = live_count[0]
        got = zip(counts.tolist()[:group], flags.tolist()[:group], costs.tolist()[:group])          # the one read of the group
        for n, (smallest, accepted), cost in got:
            if not accepted:                      # (a round that accepts nothing changes nothing: neither do those after it)
                stopped = "max_error" if smallest else "no valid collapse"
                break
            stats["rounds"] += 1
            stats["accepted"].append((faces_live - n) // 2)
            stats["max_cost"] = max(stats["max_cost"], _bits_to_float(cost))
            faces_live = n
            if faces_live <= target:              # (the rounds after it were cut to nothing)
                stopped = "target"
                break
        if stopped is None:
            ranges, corners = _live_lists(cur, V)
    # compaction: the live faces and the vertices that no collapse removed, in their order
    keep_vert = 1 - removed
    vert_off = ops.gs_scan(keep_vert)
    Vo = int(vert_off[-1].item())
    if faces_live:
        faces_out = torch.empty(faces_live, 3, dtype=torch.int32, device=f.device)
        _check(lib, lib.v3d_recon_mesh_compact_faces(cur.data_ptr(), F, V, live.data_ptr(), live_off.data_ptr(), keep_vert.data_ptr(), vert_off.data_ptr(),
                                                     faces_live, Vo, faces_out.data_ptr(), _stream()), "v3d_recon_mesh_compact_faces")
    else:
        faces_out = cur[:0].contiguous()
    kv = keep_vert.bool()
    vo, co = v[kv].contiguous(), (c[kv].contiguous() if c is not None else None)
    stats.update(faces_after=faces_live, vertices_after=Vo, reached=faces_live <= target, stopped=stopped)
    stats["boundary_vertices_after"] = int(_boundary(faces_out, Vo, *_corner_lists(faces_out, Vo)).sum()) if faces_live else 0
    return vo, faces_out, co, stats
