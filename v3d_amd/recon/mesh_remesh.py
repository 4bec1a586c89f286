"""Remesh a mesh isotropically on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshremesh.hip, include/v3d_recon.h "Mesh remeshing"):
split the long edges, collapse the short ones, flip towards valence 6, relax the vertices in their tangent planes and put them back on the
input surface - what the reference's fit_mesh does with clean_mesh(..., remesh=True, remesh_size=0.01) before it decimates and every 512
steps of its vertex fit.  Even triangles give the per-face atlas of mesh_texture.py an even texel density.

    verts, faces, colors, stats = remesh_mesh(verts, faces, colors, target_faces=50000)

    state = RemeshState(verts, faces, colors, spare=1024)                 # the steps of one round, for the tests
    keys, targets = split_propose(state, L) | collapse_propose(state, L) | flip_propose(state)
    accept, flags = select(state, keys)
    split_apply(state, accept, targets) | collapse_apply(state, accept, targets) | flip_apply(state, accept, targets)
    relax_vertices(state, 0.5); project_vertices(state, bvh, src_colors)

Only interior manifold edges are edited: open edges keep their vertices, bit for bit, and their edges.  The selection is mesh_decimate.py's;
the vertex -> corner lists are mesh_clean.py's, rebuilt every round from the live faces; every kernel has one owner per output and there are
no atomics: two calls with the same arguments return bit-equal results.  Everything runs under no_grad.  There is no fallback: without the
libraries this raises.  V = 0 and F = 0 are answered without a launch."""
from __future__ import annotations

import math
import time

import numpy as np
import torch

from ..ops import get_ops
from .geometry import _check, _stream, load_library
from .mesh_clean import INT32_MAX, _boundary, _count_arg, _mesh_arg
from .mesh_decimate import DEFAULT_MAX_VALENCE, ROUND_GROUP, _live_lists, _select, _valence_arg

PASSES = ("split", "collapse", "flip")
MIN_SPARE = 256                    # spare vertex rows (two face rows each) a run starts with at least, and grows by at least
SPARE_SHARE = 0.5                  # .. and as a share of the input's faces: a first split pass at the default edge needs about a third
MEASURES = ("edges_in_range", "area_cov", "area_ratio", "mean_min_angle", "valence6")


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def _edge_arg(value, who: str) -> float:
    e = float(np.float32(value))
    if not (e > 0 and math.isfinite(e)):
        raise ValueError(f"{who}: target_edge {value} must be positive and finite")
    return e


def _lambda_arg(value, who: str) -> float:
    lam = float(value)
    if not 0 <= lam <= 1:
        raise ValueError(f"{who}: relax {value} outside 0 .. 1")
    return lam


def default_edge(area: float, faces: int) -> float:
    """L = sqrt(4 A / (sqrt(3) F)): the edge of the equilateral triangle that F of cover the area A"""
    return math.sqrt(4.0 * area / (math.sqrt(3.0) * faces))


def mesh_measures(verts, faces) -> dict:
    """How even a mesh is (host, float64).  With L the edge of the equilateral triangle of the mean face area: "edges_in_range", the share of
    the edges within [4/5 L, 4/3 L];  "area_cov", std / mean of the face areas;  "area_ratio", largest / smallest;  "mean_min_angle", the mean
    over the faces of the smallest angle in degrees;  "valence6", the share of the vertices with faces that have 6.  nan without faces."""
    p = (verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)).astype(np.float64).reshape(-1, 3)
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return {k: float("nan") for k in MEASURES}
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    L = default_edge(float(area.sum()), f.shape[0])
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    ln = np.linalg.norm(p[e[:, 0]] - p[e[:, 1]], axis=1)
    la, lb, lc = np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1), np.linalg.norm(b - a, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.stack([(lb ** 2 + lc ** 2 - la ** 2) / (2 * lb * lc), (la ** 2 + lc ** 2 - lb ** 2) / (2 * la * lc),
                        (la ** 2 + lb ** 2 - lc ** 2) / (2 * la * lb)], 1)
    ang = np.degrees(np.arccos(np.clip(np.nan_to_num(cos, nan=1.0), -1.0, 1.0)))
    val = np.bincount(f.reshape(-1))
    val = val[val > 0]
    mean = float(area.mean())
    return {"edges_in_range": float(((ln >= 0.8 * L) & (ln <= 4.0 / 3.0 * L)).mean()), "area_cov": float(area.std() / mean) if mean > 0 else float("nan"),
            "area_ratio": float(area.max() / area.min()) if area.min() > 0 else float("inf"), "mean_min_angle": float(ang.min(1).mean()),
            "valence6": float((val == 6).mean())}


# ---- the state ------------------------------------------------------------------------------------------------------------------------------
class RemeshState:
    """THE STATE of include/v3d_recon.h "Mesh remeshing" on the device: verts, colors [Vcap, 3] float32, faces [Fcap, 3] int32 (Vcap Vcap Vcap
    for a dead or unborn face), counts [2] int32 = (V_live, F_live), removed [Vcap] int32.  `faces` may hold any int32 (an index outside the
    vertices makes a face absent)."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor, spare: int):
        V, F, dev = verts.shape[0], faces.shape[0], verts.device
        self.Vcap, self.Fcap = V + spare, F + 2 * spare
        if self.Vcap > INT32_MAX - 1 or 3 * self.Fcap > INT32_MAX:
            raise ValueError(f"RemeshState: {self.Vcap} vertex rows and {self.Fcap} face rows do not fit int32")
        self.verts = torch.zeros(self.Vcap, 3, dtype=torch.float32, device=dev)
        self.colors = torch.zeros(self.Vcap, 3, dtype=torch.float32, device=dev)
        self.faces = torch.full((self.Fcap, 3), self.Vcap, dtype=torch.int32, device=dev)
        self.verts[:V], self.colors[:V], self.faces[:F] = verts, colors, faces
        self.counts = torch.tensor([V, F], dtype=torch.int32, device=dev)
        self.removed = torch.zeros(self.Vcap, dtype=torch.int32, device=dev)
        self._lists = None

    def lists(self):
        """(ranges, corners) of the live faces, built once per state of the faces"""
        if self._lists is None:
            self._lists = _live_lists(self.faces, self.Vcap)
        return self._lists

    def touched(self):
        self._lists = None

    def grow(self, spare: int):
        """`spare` more vertex rows and twice as many face rows; the dead faces are renamed to the new Vcap"""
        old = self.Vcap
        grown = RemeshState(self.verts, torch.where(self.faces >= old, old + spare, self.faces).to(torch.int32), self.colors, spare)
        grown.counts = self.counts
        grown.removed[:old] = self.removed
        self.__dict__.update(grown.__dict__)


def _args(st: RemeshState):
    ranges, corners = st.lists()
    return ranges.data_ptr(), corners.data_ptr()


def _outputs(st: RemeshState):
    return torch.empty(st.Vcap, dtype=torch.int64, device=st.verts.device), torch.empty(st.Vcap, dtype=torch.int32, device=st.verts.device)


# ---- the steps of a round ---------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def split_propose(st: RemeshState, target_edge: float, max_valence: int = DEFAULT_MAX_VALENCE):
    """(keys [Vcap] int64, targets [Vcap] int32): every vertex's longest editable edge above 4/3 target_edge (v3d_recon_remesh_split_propose)"""
    lib = load_library()
    keys, targets = _outputs(st)
    _check(lib, lib.v3d_recon_remesh_split_propose(st.verts.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, *_args(st), target_edge, max_valence,
                                                   keys.data_ptr(), targets.data_ptr(), _stream()), "v3d_recon_remesh_split_propose")
    return keys, targets


@torch.no_grad()
def collapse_propose(st: RemeshState, target_edge: float, max_valence: int = DEFAULT_MAX_VALENCE):
    """(keys, targets): every removable vertex's shortest valid collapse below 4/5 target_edge (v3d_recon_remesh_collapse_propose)"""
    lib = load_library()
    keys, targets = _outputs(st)
    _check(lib, lib.v3d_recon_remesh_collapse_propose(st.verts.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, *_args(st), target_edge, max_valence,
                                                      keys.data_ptr(), targets.data_ptr(), _stream()), "v3d_recon_remesh_collapse_propose")
    return keys, targets


@torch.no_grad()
def boundary(st: RemeshState) -> torch.Tensor:
    return _boundary(st.faces, st.Vcap, *st.lists())


@torch.no_grad()
def flip_propose(st: RemeshState, max_valence: int = DEFAULT_MAX_VALENCE, flags=None):
    """(keys, targets): every vertex's best valence-improving flip (v3d_recon_remesh_flip_propose); flags: boundary(st) when None"""
    lib = load_library()
    flags = boundary(st) if flags is None else flags
    keys, targets = _outputs(st)
    _check(lib, lib.v3d_recon_remesh_flip_propose(st.verts.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, *_args(st), flags.data_ptr(), max_valence,
                                                  keys.data_ptr(), targets.data_ptr(), _stream()), "v3d_recon_remesh_flip_propose")
    return keys, targets


@torch.no_grad()
def select(st: RemeshState, keys: torch.Tensor, flags=None):
    """(accept [Vcap] int32, flags [2] int32 on the device): mesh_decimate's selection with no cost limit"""
    flags = torch.zeros(2, dtype=torch.int32, device=keys.device) if flags is None else flags
    accept, _, _ = _select(st.faces, st.Vcap, *st.lists(), keys, math.inf, flags)
    return accept, flags


@torch.no_grad()
def split_apply(st: RemeshState, accept, targets, flag=None, rank=None):
    """Applies the accepted splits in place, moves st.counts; flag [1] int32 on the device is set when the capacity dropped some"""
    lib, ops = load_library(), get_ops()
    flag = torch.zeros(1, dtype=torch.int32, device=accept.device) if flag is None else flag
    rank = ops.gs_scan(accept) if rank is None else rank
    counts = torch.empty_like(st.counts)
    _check(lib, lib.v3d_recon_remesh_split_apply(st.verts.data_ptr(), st.colors.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, *_args(st),
                                                 accept.data_ptr(), targets.data_ptr(), rank.data_ptr(), st.counts.data_ptr(), counts.data_ptr(),
                                                 flag.data_ptr(), _stream()), "v3d_recon_remesh_split_apply")
    st.counts = counts
    st.touched()
    return flag


@torch.no_grad()
def collapse_apply(st: RemeshState, accept, targets):
    lib = load_library()
    _check(lib, lib.v3d_recon_remesh_collapse_apply(st.faces.data_ptr(), st.Fcap, st.Vcap, *_args(st), accept.data_ptr(), targets.data_ptr(),
                                                    st.removed.data_ptr(), _stream()), "v3d_recon_remesh_collapse_apply")
    st.touched()


@torch.no_grad()
def flip_apply(st: RemeshState, accept, targets):
    lib = load_library()
    _check(lib, lib.v3d_recon_remesh_flip_apply(st.faces.data_ptr(), st.Fcap, st.Vcap, *_args(st), accept.data_ptr(), targets.data_ptr(), _stream()),
           "v3d_recon_remesh_flip_apply")
    st.touched()


@torch.no_grad()
def relax_vertices(st: RemeshState, lam: float, pinned=None, flags=None):
    """st.verts after one tangential umbrella step (v3d_recon_remesh_relax); vertices on open edges and pinned ones stay, bit for bit"""
    lib = load_library()
    flags = boundary(st) if flags is None else flags
    out = torch.empty_like(st.verts)
    _check(lib, lib.v3d_recon_remesh_relax(st.verts.data_ptr(), st.Vcap, st.faces.data_ptr(), st.Fcap, *_args(st), flags.data_ptr(),
                                           pinned.data_ptr() if pinned is not None else None, lam, out.data_ptr(), _stream()), "v3d_recon_remesh_relax")
    st.verts = out


@torch.no_grad()
def project_vertices(st: RemeshState, bvh, src_colors: torch.Tensor):
    """Moves every vertex to the closest point of the tree's mesh and gives it the colour interpolated there (v3d_recon_bvh_closest_point,
    v3d_recon_remesh_project); bvh: mesh_bake.build_bvh of the input mesh, src_colors its vertex colours on the device"""
    from .mesh_query import closest_points
    lib = load_library()
    _, face, uv = closest_points(bvh, st.verts)
    _check(lib, lib.v3d_recon_remesh_project(face.data_ptr(), uv.data_ptr(), bvh.verts.data_ptr(), src_colors.data_ptr(), bvh.verts.shape[0],
                                             bvh.faces.data_ptr(), bvh.faces.shape[0], st.verts.data_ptr(), st.colors.data_ptr(), st.Vcap, _stream()),
           "v3d_recon_remesh_project")


# ---- the whole ------------------------------------------------------------------------------------------------------------------------------------
def _pass(st: RemeshState, op: str, L: float, max_valence: int, max_rounds, stats: dict, who: str):
    """One pass of `op`: rounds in groups of ROUND_GROUP with one read-back per group, until a round accepts nothing"""
    dev = st.verts.device
    v_live, f_live = st.counts.tolist()
    edges = 3 * f_live // 2
    limit = max_rounds if max_rounds is not None else (4 if op == "flip" else 1) * edges + 8
    rounds = ops = 0
    t0 = time.perf_counter()
    while True:
        if rounds >= limit:
            raise RuntimeError(f"{who}: the {op} pass did not end within {limit} rounds")
        group = min(ROUND_GROUP, limit - rounds)
        book = torch.zeros(group, 6, dtype=torch.int32, device=dev)          # per round: flags [2], capacity flag, accepted, counts [2]
        for j in range(group):
            if op == "split":
                keys, targets = split_propose(st, L, max_valence)
            elif op == "collapse":
                keys, targets = collapse_propose(st, L, max_valence)
            else:
                keys, targets = flip_propose(st, max_valence)
            accept, _ = select(st, keys, book[j, 0:2])
            book[j, 3] = accept.sum()
            if op == "split":
                split_apply(st, accept, targets, book[j, 2:3])
            elif op == "collapse":
                collapse_apply(st, accept, targets)
            else:
                flip_apply(st, accept, targets)
            book[j, 4:6] = st.counts
        ended = False
        for _, accepted, full, n, nv, _ in book.tolist():                     # the one read of the group
            if not accepted:                      # (a round that accepts nothing changes nothing: neither do those after it)
                ended = True
                break
            rounds += 1
            ops += (nv - v_live) if op == "split" else n
            v_live = nv
            if full:                              # the splits beyond the capacity were dropped, in this round and in those after it
                break
        if ended:
            break
        if op == "split" and bool(book[:, 2].any()):
            st.grow(max(MIN_SPARE, st.Vcap // 2))
            stats["reallocations"] += 1
    stats["operations"][op].append(ops)
    stats["rounds"][op].append(rounds)
    stats["milliseconds"][op].append(1e3 * (time.perf_counter() - t0))          # (every group ends in a read-back: the device has caught up)


@torch.no_grad()
def remesh_mesh(verts, faces, colors, *, target_edge=None, target_faces=None, iterations: int = 3, relax: float = 0.5, reproject: bool = True,
                max_valence: int = DEFAULT_MAX_VALENCE, max_rounds=None, device="cuda"):
    """(verts, faces, colors, stats) remeshed towards one edge length: `iterations` of split rounds, collapse rounds, flip rounds, one
    tangential relaxation step of factor `relax` (0: none) and, with `reproject`, the closest point of the input mesh, whose interpolated
    colour the vertex takes.  colors may be None.

    target_edge: the edge length L;  target_faces: L = sqrt(4 A / (sqrt(3) target_faces)) for the mesh's area A, the edge at which that many
    equilateral triangles cover it (the result has about that many faces, not exactly);  neither: the same at the input's own face count;  both:
    ValueError.  max_valence: a vertex with more faces proposes nothing, no collapse or flip may lift one above it.  max_rounds: RuntimeError
    when a pass takes that many rounds (None: E + 8 for split and collapse, 4 E + 8 for flip, E the pass's edge count; no pass can need them).

    Vertices on open edges keep their positions, bit for bit, and open edges stay.  Input vertices that no face uses stay.
    stats (json.dumps takes it): "target_edge", "operations", "rounds" and "milliseconds" (per pass, one figure per iteration), "reallocations", "before" /
    "after" (mesh_measures), "vertices_before" / "faces_before" / "vertices_after" / "faces_after", "distance" (mesh_query.mesh_distance to
    the input: "hausdorff" and "chamfer" over the input's diagonal), "seconds"."""
    who = "remesh_mesh"
    if target_edge is not None and target_faces is not None:
        raise ValueError(f"{who}: give target_edge or target_faces, not both")
    if target_edge is not None:
        target_edge = _edge_arg(target_edge, who)
    if target_faces is not None:
        target_faces = _count_arg(target_faces, who, "target_faces")
        if target_faces == 0:
            raise ValueError(f"{who}: target_faces must be positive")
    iterations = _count_arg(iterations, who, "iterations")
    lam = _lambda_arg(relax, who)
    max_valence = _valence_arg(max_valence, who)
    if max_rounds is not None:
        max_rounds = _count_arg(max_rounds, who, "max_rounds")
    v, f, c = _mesh_arg(verts, faces, colors, device, who)
    V, F = v.shape[0], f.shape[0]
    stats = {"target_edge": target_edge, "operations": {p: [] for p in PASSES}, "rounds": {p: [] for p in PASSES},
             "milliseconds": {p: [] for p in PASSES}, "reallocations": 0,
             "vertices_before": V, "faces_before": F, "vertices_after": V, "faces_after": F, "before": None, "after": None, "distance": None,
             "seconds": 0.0}
    if V == 0 or F == 0:
        return v, f, c, stats
    t0 = time.perf_counter()
    lib, ops = load_library(), get_ops()
    stats["before"] = mesh_measures(v, f)
    if target_edge is None:
        tri = v.double()[f.long()]
        area = float(0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1).sum())
        if not area > 0:
            raise ValueError(f"{who}: the mesh has no area: give target_edge")
        target_edge = _edge_arg(default_edge(area, target_faces or F), who)
        stats["target_edge"] = target_edge
    src_colors = c if c is not None else torch.zeros_like(v)
    st = RemeshState(v, f, src_colors, max(MIN_SPARE, int(SPARE_SHARE * F)))
    bvh = None
    if reproject and iterations:
        from .mesh_bake import build_bvh
        bvh = build_bvh(v, f, device)
    for _ in range(iterations):
        for op in PASSES:
            _pass(st, op, target_edge, max_valence, max_rounds, stats, who)
        if lam > 0:
            relax_vertices(st, lam)
        if bvh is not None:
            project_vertices(st, bvh, src_colors)
    # compaction: the live faces and the born vertices that no collapse removed, in their order
    v_live, f_live = st.counts.tolist()
    rows_v = torch.arange(st.Vcap, device=v.device)
    keep_vert = ((rows_v < v_live) & (st.removed == 0)).to(torch.int32)
    keep_face = (((st.faces >= 0) & (st.faces < st.Vcap)).all(1) & (torch.arange(st.Fcap, device=v.device) < f_live)).to(torch.int32)
    face_off, vert_off = ops.gs_scan(keep_face), ops.gs_scan(keep_vert)
    Fo, Vo = int(face_off[-1].item()), int(vert_off[-1].item())
    if Fo:
        faces_out = torch.empty(Fo, 3, dtype=torch.int32, device=v.device)
        _check(lib, lib.v3d_recon_mesh_compact_faces(st.faces.data_ptr(), st.Fcap, st.Vcap, keep_face.data_ptr(), face_off.data_ptr(), keep_vert.data_ptr(),
                                                     vert_off.data_ptr(), Fo, Vo, faces_out.data_ptr(), _stream()), "v3d_recon_mesh_compact_faces")
    else:
        faces_out = f[:0].contiguous()
    kv = keep_vert.bool()
    vo, co = st.verts[kv].contiguous(), (st.colors[kv].contiguous() if c is not None else None)
    stats.update(vertices_after=Vo, faces_after=Fo, after=mesh_measures(vo, faces_out))
    if Fo:
        from .mesh_query import mesh_distance
        d = mesh_distance(vo, faces_out, v, f, device=device)
        stats["distance"] = {"hausdorff": d["relative"]["hausdorff"], "chamfer": d["relative"]["chamfer"], "diagonal": d["diagonal"]}
    torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    return vo, faces_out, co, stats
