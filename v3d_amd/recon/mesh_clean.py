"""Clean the extracted mesh on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshtopo.hip, include/v3d_recon.h "Mesh topology"): drop the
small connected components (floaters) and the vertices that no face uses, smooth the voxel-scale noise away (Taubin), and look at the geometry
alone through its normals - what the reference's mesh stage does in Mesh.load(clean=.., renormal=True) and render_normal.

    ranges, corners = vertex_corners(faces, V)                 # the vertex -> incident-corner lists everything below walks
    normals = vertex_normals(verts, faces)
    labels, rounds = vertex_components(faces, V)
    verts, faces, colors, stats = filter_components(verts, faces, colors, min_faces=64)
    verts = taubin_smooth(verts, faces, iterations=10)
    verts, faces, colors, stats = clean_mesh(verts, faces, colors)          # filter, then smooth
    out = render_mesh_normals(cam, verts, faces)               # {"render": the normals as colours, ...}

The lists are built with v3d_gs_radix_sort_pairs (stable) and v3d_recon_mesh_vertex_ranges; every kernel is a gather with one owner per
output, no atomics: two calls with the same arguments return bit-equal results.  Everything runs under no_grad.  There is no fallback:
without the libraries this raises.  A mesh with V = 0 or F = 0 is answered without a launch."""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ops import get_ops
from .cameras import Camera, orbit_cameras
from .geometry import _check, _stream, load_library
from .mesh_render import _bg, _check_view, _render_views

INT32_MAX = 2 ** 31 - 1
ROUND_GROUP = 8                    # labelling rounds between two reads of the change flags
DEFAULT_NORMAL = (0.0, 0.0, 1.0)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def _tensor(a) -> torch.Tensor:
    return a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def _faces_arg(faces, num_verts: int, device, who: str) -> torch.Tensor:
    """faces [F, 3] int32 on `device`; a ValueError for anything that is not an integer [F, 3] array with indices in 0 .. V-1"""
    f = _tensor(faces)
    if f.is_floating_point() or f.is_complex() or f.dtype == torch.bool:
        raise ValueError(f"{who}: faces must be integers, got {f.dtype}")
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{who}: faces must be [F, 3], got {tuple(f.shape)}")
    if int(num_verts) < 0:
        raise ValueError(f"{who}: num_verts {num_verts} must not be negative")
    if 3 * f.shape[0] > INT32_MAX:
        raise ValueError(f"{who}: {f.shape[0]} faces: 3 F must not exceed {INT32_MAX}")
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= int(num_verts)):
        raise ValueError(f"{who}: face index outside the vertex array")
    return f.to(device=device, dtype=torch.int32).contiguous()


def _rows_arg(a, device, who: str, what: str) -> torch.Tensor:
    t = _tensor(a)
    if not t.is_floating_point():
        raise ValueError(f"{who}: {what} must be floating point, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: {what} must be [V, 3], got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).contiguous()


def _mesh_arg(verts, faces, colors, device, who: str):
    v = _rows_arg(verts, device, who, "verts")
    c = None
    if colors is not None:
        c = _rows_arg(colors, device, who, "colors")
        if c.shape != v.shape:
            raise ValueError(f"{who}: {v.shape[0]} vertices, {c.shape[0]} colours")
    return v, _faces_arg(faces, v.shape[0], device, who), c


def _count_arg(value, who: str, name: str) -> int:
    if isinstance(value, bool) or int(value) != value or int(value) < 0:
        raise ValueError(f"{who}: {name} {value} must be an integer that is not negative")
    return int(value)


# ---- the kernels, on validated device tensors (V >= 1, F >= 1) ------------------------------------------------------------------------------
def _corner_lists(f: torch.Tensor, V: int):
    lib, ops = load_library(), get_ops()
    F = f.shape[0]
    keys = torch.empty(3 * F, dtype=torch.int64, device=f.device)
    vals = torch.empty(3 * F, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_corner_records(f.data_ptr(), F, V, keys.data_ptr(), vals.data_ptr(), _stream()), "v3d_recon_mesh_corner_records")
    keys_s, corners = ops.gs_radix_sort_pairs(keys, vals, max(1, (V - 1).bit_length()))
    ranges = torch.empty(V, 2, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_vertex_ranges(keys_s.data_ptr(), 3 * F, V, ranges.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
    return ranges, corners


def _normals(v, f, ranges, corners):
    lib = load_library()
    out = torch.empty_like(v)
    _check(lib, lib.v3d_recon_mesh_vertex_normals(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(),
                                                  out.data_ptr(), _stream()), "v3d_recon_mesh_vertex_normals")
    return out


def _labels(f, V: int, ranges, corners):
    """(labels [V] int32, rounds): rounds counts up to and including the first round that changed nothing.  The rounds run in groups of
    ROUND_GROUP, each with a flag word of its own, and the flags are read once per group."""
    lib = load_library()
    cur = torch.arange(V, dtype=torch.int32, device=f.device)
    nxt = torch.empty_like(cur)
    flags = torch.empty(ROUND_GROUP, dtype=torch.int32, device=f.device)
    done, limit = 0, V + 8
    while done < limit:
        group = min(ROUND_GROUP, limit - done)
        flags.zero_()
        for j in range(group):
            _check(lib, lib.v3d_recon_mesh_label_round(f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(), V, cur.data_ptr(),
                                                       nxt.data_ptr(), flags.data_ptr() + 4 * j, _stream()), "v3d_recon_mesh_label_round")
            cur, nxt = nxt, cur
        changed = flags.cpu().tolist()[:group]
        if 0 in changed:                         # the rounds after it changed nothing either: `cur` is the fixed point
            return cur, done + changed.index(0) + 1
        done += group
    raise RuntimeError(f"vertex_components: no fixed point after {limit} rounds on {V} vertices: the corner lists are broken")


def _sorted_counts(keys: torch.Tensor, vals: torch.Tensor, V: int, nbits: int) -> torch.Tensor:
    """How many keys equal every v in 0 .. V-1, through the sort and v3d_recon_mesh_vertex_ranges"""
    lib, ops = load_library(), get_ops()
    keys_s, _ = ops.gs_radix_sort_pairs(keys, vals, nbits)
    r = torch.empty(V, 2, dtype=torch.int32, device=keys.device)
    _check(lib, lib.v3d_recon_mesh_vertex_ranges(keys_s.data_ptr(), keys.numel(), V, r.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
    return r[:, 1] - r[:, 0]


def _component_table(f, V: int, labels) -> list:
    """[{"root", "faces", "vertices"}] of the components that have a face, by ascending root"""
    lib = load_library()
    F = f.shape[0]
    keys = torch.empty(F, dtype=torch.int64, device=f.device)
    vals = torch.empty(F, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_face_labels(f.data_ptr(), F, labels.data_ptr(), V, keys.data_ptr(), vals.data_ptr(), _stream()),
           "v3d_recon_mesh_face_labels")
    nfaces = _sorted_counts(keys, vals, V, max(1, V.bit_length()))
    nverts = _sorted_counts(labels.to(torch.int64), torch.arange(V, dtype=torch.int32, device=f.device), V, max(1, (V - 1).bit_length()))
    roots = torch.nonzero(nfaces > 0).reshape(-1)
    return [{"root": r, "faces": nf, "vertices": nv} for r, nf, nv in zip(roots.tolist(), nfaces[roots].tolist(), nverts[roots].tolist())]


def kept_roots(table: list, min_faces: int = 64, keep_largest: int = 0) -> list:
    """The roots of the components of `table` that stay, ascending: those with at least min_faces faces and, with keep_largest = K > 0, among
    them the K with the most faces (ties go to the smaller root)."""
    rows = [r for r in table if r["faces"] >= min_faces]
    if keep_largest > 0:
        rows = sorted(rows, key=lambda r: (-r["faces"], r["root"]))[:keep_largest]
    return sorted(r["root"] for r in rows)


def _compact(v, f, c, ranges, corners, labels, roots: list):
    """(verts, faces, colors, vert_off [V + 1]) with only the components of `roots` (at least one), in their original order"""
    lib, ops = load_library(), get_ops()
    V, F = v.shape[0], f.shape[0]
    keep_root = torch.zeros(V, dtype=torch.int32, device=f.device)
    keep_root[torch.tensor(roots, dtype=torch.long, device=f.device)] = 1
    keep_face = torch.empty(F, dtype=torch.int32, device=f.device)
    keep_vert = torch.empty(V, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_keep_flags(f.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), V, labels.data_ptr(), keep_root.data_ptr(),
                                              keep_face.data_ptr(), keep_vert.data_ptr(), _stream()), "v3d_recon_mesh_keep_flags")
    face_off, vert_off = ops.gs_scan(keep_face), ops.gs_scan(keep_vert)
    Fo, Vo = int(face_off[-1].item()), int(vert_off[-1].item())
    faces_out = torch.empty(Fo, 3, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_compact_faces(f.data_ptr(), F, V, keep_face.data_ptr(), face_off.data_ptr(), keep_vert.data_ptr(),
                                                 vert_off.data_ptr(), Fo, Vo, faces_out.data_ptr(), _stream()), "v3d_recon_mesh_compact_faces")
    kv = keep_vert.bool()
    return v[kv].contiguous(), faces_out, (c[kv].contiguous() if c is not None else None), vert_off


def _boundary(f, V: int, ranges, corners):
    lib = load_library()
    flags = torch.empty(V, dtype=torch.int32, device=f.device)
    _check(lib, lib.v3d_recon_mesh_boundary_flags(f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(), V, flags.data_ptr(), _stream()),
           "v3d_recon_mesh_boundary_flags")
    return flags


def _smooth(v, f, ranges, corners, pinned, iterations: int, lam: float, mu: float):
    lib = load_library()
    cur, nxt = v.clone(), torch.empty_like(v)
    for _ in range(iterations):
        for factor in (lam, mu):
            _check(lib, lib.v3d_recon_mesh_smooth_pass(cur.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], ranges.data_ptr(), corners.data_ptr(),
                                                       pinned.data_ptr() if pinned is not None else None, float(factor), nxt.data_ptr(), _stream()),
                   "v3d_recon_mesh_smooth_pass")
            cur, nxt = nxt, cur
    return cur


# ---- the public functions -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def vertex_corners(faces, num_verts: int, device="cuda"):
    """(ranges [V, 2] int32, corners [3F] int32): the corners corners[ranges[v, 0] : ranges[v, 1]] touch vertex v, ascending; corner 3 f + k is
    place k of face f.  0 0 for a vertex without faces."""
    f = _faces_arg(faces, num_verts, device, "vertex_corners")
    V = int(num_verts)
    if V == 0 or f.shape[0] == 0:
        return torch.zeros(V, 2, dtype=torch.int32, device=device), torch.zeros(0, dtype=torch.int32, device=device)
    return _corner_lists(f, V)


@torch.no_grad()
def vertex_normals(verts, faces, device="cuda") -> torch.Tensor:
    """normals [V, 3]: the area-weighted mean of the incident faces' normals, of length 1; (0, 0, 1) where there is none"""
    v, f, _ = _mesh_arg(verts, faces, None, device, "vertex_normals")
    if v.shape[0] == 0 or f.shape[0] == 0:
        return torch.tensor(DEFAULT_NORMAL, dtype=torch.float32, device=device).expand(v.shape[0], 3).contiguous()
    return _normals(v, f, *_corner_lists(f, v.shape[0]))


@torch.no_grad()
def vertex_components(faces, num_verts: int, device="cuda"):
    """(labels [V] int32, rounds): labels[v] = the smallest vertex index of v's connected component (two vertices are joined when a face uses
    both; a vertex without faces labels itself); rounds = how many labelling rounds ran up to and including the first that changed nothing."""
    f = _faces_arg(faces, num_verts, device, "vertex_components")
    V = int(num_verts)
    if V == 0 or f.shape[0] == 0:
        return torch.arange(V, dtype=torch.int32, device=device), 0
    return _labels(f, V, *_corner_lists(f, V))


def _empty_like_mesh(v, f, c):
    return v[:0].contiguous(), f[:0].contiguous(), (c[:0].contiguous() if c is not None else None)


def _filter(v, f, c, ranges, corners, min_faces: int, keep_largest: int):
    """filter_components on validated device tensors with their lists (V, F >= 1)"""
    V, F = v.shape[0], f.shape[0]
    labels, rounds = _labels(f, V, ranges, corners)
    before = _component_table(f, V, labels)
    roots = kept_roots(before, min_faces, keep_largest)
    stats = {"rounds": rounds, "components_before": before, "unreferenced_vertices": V - sum(r["vertices"] for r in before)}
    if roots:
        vo, fo, co, vert_off = _compact(v, f, c, ranges, corners, labels, roots)
        new_root = vert_off[torch.tensor(roots, dtype=torch.long, device=f.device)].tolist()
        rows = {r["root"]: r for r in before}
        stats["components_after"] = [{"root": n, "faces": rows[r]["faces"], "vertices": rows[r]["vertices"]} for r, n in zip(roots, new_root)]
    else:                                                   # nothing stays: no flags, no scans, no compaction
        vo, fo, co = _empty_like_mesh(v, f, c)
        stats["components_after"] = []
    stats["removed_faces"], stats["removed_vertices"] = F - fo.shape[0], V - vo.shape[0]
    return vo, fo, co, stats


@torch.no_grad()
def filter_components(verts, faces, colors, min_faces: int = 64, keep_largest: int = 0, device="cuda"):
    """(verts, faces, colors, stats) without the connected components of fewer than min_faces faces, without all but the keep_largest
    components of the most faces (0: off; ties go to the smaller root), and without the vertices that no face uses.  What stays keeps its
    order: a mesh with nothing to remove comes back bit-equal.  stats: "components_before" / "components_after" ([{"root", "faces",
    "vertices"}] of the components that have a face), "removed_faces", "removed_vertices", "unreferenced_vertices", "rounds"."""
    min_faces = _count_arg(min_faces, "filter_components", "min_faces")
    keep_largest = _count_arg(keep_largest, "filter_components", "keep_largest")
    v, f, c = _mesh_arg(verts, faces, colors, device, "filter_components")
    V, F = v.shape[0], f.shape[0]
    if V == 0 or F == 0:
        vo, fo, co = _empty_like_mesh(v, f, c)
        return vo, fo, co, {"rounds": 0, "components_before": [], "components_after": [], "unreferenced_vertices": V, "removed_faces": F,
                            "removed_vertices": V}
    return _filter(v, f, c, *_corner_lists(f, V), min_faces, keep_largest)


@torch.no_grad()
def boundary_vertices(faces, num_verts: int, device="cuda") -> torch.Tensor:
    """flags [V] int32: 1 where the vertex lies on an open edge (one of its neighbours shares exactly one face with it)"""
    f = _faces_arg(faces, num_verts, device, "boundary_vertices")
    V = int(num_verts)
    if V == 0 or f.shape[0] == 0:
        return torch.zeros(V, dtype=torch.int32, device=device)
    return _boundary(f, V, *_corner_lists(f, V))


def _smooth_args(iterations, lam, mu, who: str):
    iterations = _count_arg(iterations, who, "iterations")
    if not (math.isfinite(float(lam)) and math.isfinite(float(mu))):
        raise ValueError(f"{who}: lam {lam} and mu {mu} must be finite")
    return iterations, float(lam), float(mu)


@torch.no_grad()
def taubin_smooth(verts, faces, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, fix_boundary: bool = False, device="cuda") -> torch.Tensor:
    """verts [V, 3] after `iterations` pairs of umbrella passes with the factors lam, then mu (Taubin: the second, negative pass undoes the
    shrinkage of the first).  With fix_boundary the vertices on open edges (boundary_vertices) stay where they are, bit for bit; a vertex
    without faces always does."""
    iterations, lam, mu = _smooth_args(iterations, lam, mu, "taubin_smooth")
    v, f, _ = _mesh_arg(verts, faces, None, device, "taubin_smooth")
    if v.shape[0] == 0 or f.shape[0] == 0 or iterations == 0:
        return v.clone()
    ranges, corners = _corner_lists(f, v.shape[0])
    pinned = _boundary(f, v.shape[0], ranges, corners) if fix_boundary else None
    return _smooth(v, f, ranges, corners, pinned, iterations, lam, mu)


@torch.no_grad()
def clean_mesh(verts, faces, colors, min_faces: int = 64, keep_largest: int = 0, iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
               fix_boundary: bool = False, device="cuda"):
    """(verts, faces, colors, stats): filter_components, then taubin_smooth; the colours ride along.  min_faces = 0 with keep_largest = 0 leaves
    the filter out (unreferenced vertices then stay), iterations = 0 the smoothing.  stats (plain ints, lists and dicts: json.dumps takes it):
    the filter's, "vertices" / "faces" and "vertices_before" / "faces_before", "boundary_vertices_before" / "boundary_vertices_after",
    "filtered", "smooth_iterations"."""
    min_faces = _count_arg(min_faces, "clean_mesh", "min_faces")
    keep_largest = _count_arg(keep_largest, "clean_mesh", "keep_largest")
    iterations, lam, mu = _smooth_args(iterations, lam, mu, "clean_mesh")
    v, f, c = _mesh_arg(verts, faces, colors, device, "clean_mesh")
    V, F = v.shape[0], f.shape[0]
    filtered = bool(min_faces or keep_largest)
    stats = {"vertices_before": V, "faces_before": F, "filtered": filtered, "smooth_iterations": iterations, "boundary_vertices_before": 0,
             "boundary_vertices_after": 0}
    if V == 0 or F == 0:
        vo, fo, co = (_empty_like_mesh(v, f, c) if filtered else (v, f, c))
        stats.update({"rounds": 0, "components_before": [], "components_after": [], "unreferenced_vertices": V, "removed_faces": 0,
                      "removed_vertices": V - vo.shape[0]})
    else:
        ranges, corners = _corner_lists(f, V)
        stats["boundary_vertices_before"] = int(_boundary(f, V, ranges, corners).sum())
        if filtered:
            vo, fo, co, fstats = _filter(v, f, c, ranges, corners, min_faces, keep_largest)
            stats.update(fstats)
            if fo.shape[0] and (fstats["removed_faces"] or fstats["removed_vertices"]):
                ranges, corners = _corner_lists(fo, vo.shape[0])
        else:
            labels, rounds = _labels(f, V, ranges, corners)
            table = _component_table(f, V, labels)
            vo, fo, co = v, f, c
            stats.update({"rounds": rounds, "components_before": table, "components_after": table, "removed_faces": 0, "removed_vertices": 0,
                          "unreferenced_vertices": V - sum(r["vertices"] for r in table)})
        if fo.shape[0]:
            pinned = _boundary(fo, vo.shape[0], ranges, corners)
            stats["boundary_vertices_after"] = int(pinned.sum())
            if iterations:
                vo = _smooth(vo, fo, ranges, corners, pinned if fix_boundary else None, iterations, lam, mu)
    stats["vertices"], stats["faces"] = vo.shape[0], fo.shape[0]
    return vo, fo, co, stats


# ---- normals as colours -----------------------------------------------------------------------------------------------------------------------
def normal_colors(camera: Camera, normals: torch.Tensor) -> torch.Tensor:
    """[V, 3] in 0 .. 1: (n + 1) / 2 of the normals in the camera's frame with x right, y up and z TOWARDS the camera, so a surface that
    faces the camera is (0.5, 0.5, 1).  The rotation is camera.world_view's (row vectors; its view axes are x right, y down, z forward)."""
    R = camera.world_view[:3, :3].to(device=normals.device, dtype=torch.float32)
    flip = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float32, device=normals.device)
    return ((normals @ R) * flip + 1.0) * 0.5


@torch.no_grad()
def render_mesh_normals(camera: Camera, verts, faces, normals=None, bg=(1.0, 1.0, 1.0), cull: bool = True, device="cuda") -> dict:
    """render_mesh's dict of the mesh with its camera-space normals (normal_colors; vertex_normals when `normals` is None) as vertex colours,
    over `bg`: the reference's render_normal.  No raster kernel of its own."""
    _check_view(int(camera.width), int(camera.height), 8)
    v, f, n = _mesh_arg(verts, faces, normals, device, "render_mesh_normals")
    if n is None:
        n = _normals(v, f, *_corner_lists(f, v.shape[0])) if v.shape[0] and f.shape[0] else torch.zeros_like(v)
    return _render_views(camera, v, f, normal_colors(camera, n).contiguous(), list(bg), ((cull, False),))[0]


@torch.no_grad()
def render_normal_orbit(verts, faces, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool = True,
                        cull: bool = True, normals=None, device="cuda") -> np.ndarray:
    """n turntable frames of the normals (render_mesh_normals) from the cameras of orbit_cameras, uint8 [n, reso, reso, 3] on the host"""
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    _check_view(int(reso), int(reso), 8)
    v, f, nrm = _mesh_arg(verts, faces, normals, device, "render_normal_orbit")
    if nrm is None:
        nrm = _normals(v, f, *_corner_lists(f, v.shape[0])) if v.shape[0] and f.shape[0] else torch.zeros_like(v)
    out = []
    for cam in cams:
        img = _render_views(cam, v, f, normal_colors(cam, nrm).contiguous(), _bg(white_background), ((cull, False),))[0]["render"]
        out.append((img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu())
    return torch.stack(out).numpy() if out else np.zeros((0, int(reso), int(reso), 3), dtype=np.uint8)
