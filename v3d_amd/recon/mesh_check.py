"""Is the mesh sound: closed, manifold, consistently wound and free of faces that pass through each other, on the gfx950 kernels of
libv3d_recon.so (csrc_recon/meshcheck.hip, include/v3d_recon.h "Mesh check"): a walk of the BVH of mesh_bake.py with the mesh's own faces
as queries, and a census of the faces at every edge on the corner lists of mesh_clean.py.

    bvh = mesh_bake.build_bvh(verts, faces)
    hits = self_intersections(bvh)                       # {"pairs" [n, 2] int32 sorted, f < g; "per_face" [F] int32; "count"}
    same, opposite, flags = edge_census(faces, V)        # per half-edge [3F], [3F]; per vertex [V] (bits 1 open, 2 non-manifold, 4 winding, 8 pinched)
    report = check_mesh(verts, faces)                    # a dict of plain numbers; report["watertight"]

Unlike the other stages' meshes this one may hold faces with an index outside the vertices (absent: counted, and ignored by everything
else), faces that name a vertex twice and faces without area.  No atomics anywhere: two calls with the same arguments return bit-equal
results.  Everything runs under no_grad.  There is no fallback: without the libraries this raises."""
from __future__ import annotations

import time

import numpy as np
import torch

from ..ops import get_ops
from .geometry import _check, _stream, load_library
from .mesh_bake import MeshBVH, _high_mesh, build_bvh
from .mesh_clean import _corner_lists, vertex_components
from .mesh_query import _int_arg

INT32_MAX = 2 ** 31 - 1
DEFAULT_MAX_PAIRS = 1 << 24
OPEN, NON_MANIFOLD, WINDING, PINCHED = 1, 2, 4, 8          # the bits of v3d_recon_mesh_vertex_census


# ---- the pairs ------------------------------------------------------------------------------------------------------------------------------
def _self_count(bvh: MeshBVH):
    lib = load_library()
    F, dev = bvh.num_faces, bvh.verts.device
    n_all = torch.empty(F, dtype=torch.int32, device=dev)
    n_up = torch.empty(F, dtype=torch.int32, device=dev)
    _check(lib, lib.v3d_recon_bvh_self_count(*bvh._args(), n_all.data_ptr(), n_up.data_ptr(), _stream()), "v3d_recon_bvh_self_count")
    return n_all, n_up


def _self_emit(bvh: MeshBVH, offsets: torch.Tensor, total: int):
    lib = load_library()
    pairs = torch.empty(total, 2, dtype=torch.int32, device=bvh.verts.device)
    _check(lib, lib.v3d_recon_bvh_self_emit(*bvh._args(), offsets.data_ptr(), total, pairs.data_ptr(), _stream()), "v3d_recon_bvh_self_emit")
    return pairs


def _sort_pairs(pairs: torch.Tensor, F: int):
    """by (f, g): v3d_gs_radix_sort_pairs on f << 32 | g"""
    keys = (pairs[:, 0].to(torch.int64) << 32) | pairs[:, 1].to(torch.int64)
    vals = torch.arange(pairs.shape[0], dtype=torch.int32, device=pairs.device)
    keys_s, _ = get_ops().gs_radix_sort_pairs(keys.contiguous(), vals, 32 + max(1, (F - 1).bit_length()))
    return torch.stack([keys_s >> 32, keys_s & 0xFFFFFFFF], 1).to(torch.int32)


@torch.no_grad()
def self_intersections(bvh: MeshBVH, max_pairs: int = DEFAULT_MAX_PAIRS, timings: dict = None) -> dict:
    """The pairs of faces of the tree's mesh that pass through each other by THE PAIR RULE of include/v3d_recon.h.  "pairs": [n, 2] int32 on
    the tree's device, f < g, sorted by (f, g);  "per_face": [F] int32, the partners of every face in either index order;  "count": n.
    With more than max_pairs (1 .. 2^31 - 1) pairs the list is not written: "pairs" is None and the counts stand.  The total is summed in
    int64 on the host and the scan runs only when it is at most max_pairs, so no scan total passes int32.  timings, when given, receives the
    seconds of "count", "scan", "emit" and "sort" (each ended by a synchronize)."""
    if not isinstance(bvh, MeshBVH):
        raise ValueError(f"self_intersections: bvh must be a MeshBVH of build_bvh, got {type(bvh).__name__}")
    cap = _int_arg(max_pairs, 1, INT32_MAX, "self_intersections", "max_pairs")
    F = bvh.num_faces

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[name] = time.perf_counter() - t0
        return time.perf_counter()

    t = time.perf_counter()
    n_all, n_up = _self_count(bvh)
    total = int(n_up.sum(dtype=torch.int64))
    t = lap("count", t)
    out = {"pairs": None, "per_face": n_all, "count": total}
    if total > cap:
        return out
    if total == 0:
        out["pairs"] = torch.empty(0, 2, dtype=torch.int32, device=bvh.verts.device)
        return out
    offsets = get_ops().gs_scan(n_up)
    t = lap("scan", t)
    pairs = _self_emit(bvh, offsets, total)
    t = lap("emit", t)
    out["pairs"] = _sort_pairs(pairs, F)
    lap("sort", t)
    return out


# ---- the census -----------------------------------------------------------------------------------------------------------------------------
def _census(f: torch.Tensor, V: int):
    """on validated device tensors (V, F >= 1, 3 F <= INT32_MAX)"""
    lib = load_library()
    F = f.shape[0]
    ranges, corners = _corner_lists(f, V)
    same = torch.empty(3 * F, dtype=torch.int32, device=f.device)
    opposite = torch.empty(3 * F, dtype=torch.int32, device=f.device)
    flags = torch.empty(V, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_edge_census(f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, same.data_ptr(), opposite.data_ptr(), _stream()),
           "v3d_recon_mesh_edge_census")
    _check(lib, lib.v3d_recon_mesh_vertex_census(f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, flags.data_ptr(), _stream()),
           "v3d_recon_mesh_vertex_census")
    return same, opposite, flags


def _census_faces(faces, num_verts, device, who: str):
    f = faces.detach() if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(faces))
    if f.is_floating_point() or f.is_complex() or f.dtype == torch.bool or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{who}: faces must be integers [F, 3], got {f.dtype} {tuple(f.shape)}")
    V = _int_arg(num_verts, 1, INT32_MAX, who, "num_verts")
    if f.shape[0] == 0:
        raise ValueError(f"{who}: no faces to count")
    if 3 * f.shape[0] > INT32_MAX:
        raise ValueError(f"{who}: {f.shape[0]} faces: 3 F must not exceed {INT32_MAX}")
    return f.clamp(-1, INT32_MAX).to(device=device, dtype=torch.int32).contiguous(), V


@torch.no_grad()
def edge_census(faces, num_verts: int, device="cuda"):
    """(same [3F], opposite [3F], flags [V]) int32 on `device`, as v3d_recon_mesh_edge_census and v3d_recon_mesh_vertex_census write them:
    for corner 3 f + k, the half-edge from place k to place k + 1 of face f, how many faces run the same way along that edge (itself included)
    and how many the other way, -1 -1 for a face with an index outside 0 .. V-1 or a repeated index;  per vertex the OR of OPEN,
    NON_MANIFOLD, WINDING, or else PINCHED."""
    f, V = _census_faces(faces, num_verts, device, "edge_census")
    return _census(f, V)


# ---- the report -----------------------------------------------------------------------------------------------------------------------------
def _count_where(mask) -> int:
    return int(mask.sum())


def build_report(verts, faces, same, opposite, flags, components: int, per_face, pair_count: int, seconds: float = 0.0) -> dict:
    """The report of check_mesh from the kernels' integer outputs (host tensors or arrays):  same, opposite [3F] and flags [V] of edge_census,
    per_face [F] and pair_count of self_intersections, components of vertex_components.  Integers stay integers;  area and volume are summed
    in float64."""
    v = torch.as_tensor(np.asarray(verts)).double().reshape(-1, 3)
    f = torch.as_tensor(np.asarray(faces)).long().reshape(-1, 3)
    same, opposite = torch.as_tensor(np.asarray(same)).long().reshape(-1), torch.as_tensor(np.asarray(opposite)).long().reshape(-1)
    flags, per_face = torch.as_tensor(np.asarray(flags)).long().reshape(-1), torch.as_tensor(np.asarray(per_face)).long().reshape(-1)
    V, F = v.shape[0], f.shape[0]
    present = ((f >= 0) & (f < V)).all(1)
    fp = f[present]
    counted = present.clone()
    counted[present] = (fp[:, 0] != fp[:, 1]) & (fp[:, 1] != fp[:, 2]) & (fp[:, 2] != fp[:, 0])
    # the area rule of the kernels: e1 x e2 == 0 with every float32 product rounded on its own
    p = torch.as_tensor(np.asarray(verts)).float().reshape(-1, 3)
    e1, e2 = p[fp[:, 1]] - p[fp[:, 0]], p[fp[:, 2]] - p[fp[:, 0]]
    flat = ((e1[:, 1] * e2[:, 2] == e1[:, 2] * e2[:, 1]) & (e1[:, 2] * e2[:, 0] == e1[:, 0] * e2[:, 2]) & (e1[:, 0] * e2[:, 1] == e1[:, 1] * e2[:, 0]))
    used = torch.zeros(V, dtype=torch.bool)
    used[f[counted].reshape(-1)] = True
    mult = (same + opposite)[same >= 0]
    by_mult = {}
    for m, n in zip(*[x.tolist() for x in torch.unique(mult, return_counts=True)]):
        if n % m:
            raise RuntimeError(f"check_mesh: {n} half-edges of multiplicity {m}: the census is not that of one mesh")
        by_mult[int(m)] = n // m
    twice = _count_where((same == 2) & (opposite == 0))
    if twice % 2:
        raise RuntimeError(f"check_mesh: {twice} half-edges run the same way in twos: the census is not that of one mesh")
    E, Fc, Vu = sum(by_mult.values()), _count_where(counted), _count_where(used)
    boundary, non_manifold, inconsistent = by_mult.get(1, 0), sum(n for m, n in by_mult.items() if m >= 3), twice // 2
    pinched = _count_where((flags & PINCHED) != 0)
    closed, manifold, oriented = Fc > 0 and boundary == 0, non_manifold == 0 and pinched == 0, inconsistent == 0
    euler = Vu - E + Fc
    a, b, c = v[fp[:, 0]], v[fp[:, 1]], v[fp[:, 2]]
    area = 0.5 * float(torch.linalg.cross(b - a, c - a).norm(dim=1).sum())
    sound = closed and manifold and oriented
    genus = None
    if sound and (2 * components - euler) % 2 == 0:
        genus = (2 * components - euler) // 2
    volume = float((a * torch.linalg.cross(b, c)).sum()) / 6.0 if closed and oriented else None
    return {"vertices": V, "vertices_used": Vu, "faces": F, "absent_faces": F - _count_where(present), "repeated_index_faces": _count_where(present) - Fc,
            "zero_area_faces": _count_where(flat), "edges": E, "edges_by_multiplicity": {str(m): n for m, n in sorted(by_mult.items())},
            "boundary_edges": boundary, "non_manifold_edges": non_manifold, "inconsistent_edges": inconsistent, "pinched_vertices": pinched,
            "components": int(components), "euler": euler, "closed": closed, "manifold": manifold, "oriented": oriented, "genus": genus, "area": area,
            "volume": volume, "self_intersections": int(pair_count), "intersecting_faces": _count_where(per_face > 0),
            "watertight": sound and int(pair_count) == 0, "seconds": float(seconds)}


def count_components(labels, faces, num_verts: int) -> int:
    """The components of vertex_components that have a face"""
    f = torch.as_tensor(np.asarray(faces)).long().reshape(-1, 3)
    present = ((f >= 0) & (f < num_verts)).all(1)
    lab = torch.as_tensor(np.asarray(labels)).long()
    return int(torch.unique(lab[f[present][:, 0]]).numel())


@torch.no_grad()
def check_mesh(verts, faces, device="cuda", max_pairs: int = DEFAULT_MAX_PAIRS, details: bool = False):
    """The report: a dict of plain numbers.  "vertices", "vertices_used" (by a counted face: present, three different indices), "faces",
    "absent_faces" (an index outside the vertices), "repeated_index_faces", "zero_area_faces" (present, no area by the kernels' rule);
    "edges" and "edges_by_multiplicity" ({"2": n, ..}: undirected edges by the number of counted faces on them);  "boundary_edges" (one
    face), "non_manifold_edges" (three or more), "inconsistent_edges" (two faces that run the same way), "pinched_vertices";  "components";
    "euler" = vertices_used - edges + counted faces;  "closed", "manifold" (no non-manifold edge, no pinched vertex), "oriented";  "genus"
    when all three hold (else None);  "area", and the signed "volume" when closed and oriented (else None), both summed in float64;
    "self_intersections" (pairs of faces) and "intersecting_faces";  "watertight": closed, manifold, oriented and no such pair;  "seconds".
    details = True returns (report, {"pairs", "per_face", "same", "opposite", "flags"}) with the tensors on `device`."""
    v, f = _high_mesh(verts, faces, device, "check_mesh")
    V, F = v.shape[0], f.shape[0]
    if 3 * F > INT32_MAX:
        raise ValueError(f"check_mesh: {F} faces: 3 F must not exceed {INT32_MAX}")
    cap = _int_arg(max_pairs, 1, INT32_MAX, "check_mesh", "max_pairs")
    t0 = time.perf_counter()
    hits = self_intersections(build_bvh(v, f, device), cap)
    same, opposite, flags = _census(f, V)
    present = ((f >= 0) & (f < V)).all(1)
    components = 0
    if bool(present.any()):
        labels, _ = vertex_components(f[present], V, device)
        components = count_components(labels.cpu(), f.cpu(), V)
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    report = build_report(v.cpu(), f.cpu(), same.cpu(), opposite.cpu(), flags.cpu(), components, hits["per_face"].cpu(), hits["count"],
                          time.perf_counter() - t0)
    if details:
        return report, {"pairs": hits["pairs"], "per_face": hits["per_face"], "same": same, "opposite": opposite, "flags": flags}
    return report
