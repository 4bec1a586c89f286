"""Restatement of the mesh repair (include/v3d_recon.h "Mesh repair", csrc_recon/meshrepair.hip, v3d_amd/recon/mesh_repair.py) in plain python:
dicts and lists, python floats (float64) and numpy float32 for the one rounding.  Every pass follows the header's rule to the letter and
nothing else;  the pair rule, the census, the report and the scenes are those of tests/mesh_check_ref.py, imported and left as they are.

repair() is the loop of repair_mesh.  Every check it runs (one per round, and the report after) notes the smallest pair-rule margin it met:
tests/test_mesh_repair_cpu.py holds every whole-loop scene to SCENE_MARGIN in every round, which makes "the float32 kernels decide like
this float64 restatement" a fair demand."""
import functools
import math

import numpy as np
import torch

import mesh_check_ref as R
import mesh_render_ref as M

DOUBLING_ROUNDS = 32
WINDING_BITS = R.NON_MANIFOLD | R.WINDING | R.PINCHED


def rows_of(faces):
    return [tuple(int(x) for x in r) for r in np.asarray(faces).reshape(-1, 3)]


def present(r, V):
    return all(0 <= i < V for i in r)


def counted(r, V):
    return present(r, V) and len(set(r)) == 3


# ---- 1. weld --------------------------------------------------------------------------------------------------------------------------------
def weld(verts):
    """remap [V]: the smallest index with the same three float32 values (0.0 == -0.0, as python compares and hashes them)"""
    v = np.asarray(verts, dtype=np.float32)
    first, remap = {}, []
    for i in range(v.shape[0]):
        remap.append(first.setdefault((float(v[i, 0]), float(v[i, 1]), float(v[i, 2])), i))
    return remap


def remap_faces(faces, remap):
    V = len(remap)
    return [tuple(remap[i] for i in r) if present(r, V) else r for r in rows_of(faces)]


# ---- 2. drop --------------------------------------------------------------------------------------------------------------------------------
def no_area(verts, r):
    v = np.asarray(verts, dtype=np.float32)
    e1, e2 = v[r[1]] - v[r[0]], v[r[2]] - v[r[0]]               # float32 differences, every product rounded to float32
    return bool(e1[1] * e2[2] == e1[2] * e2[1] and e1[2] * e2[0] == e1[0] * e2[2] and e1[0] * e2[1] == e1[1] * e2[0])


def drop_bits(verts, faces):
    V = np.asarray(verts).shape[0]
    seen, out = set(), []
    for r in rows_of(faces):
        if not present(r, V):
            out.append(1)
            continue
        bits = (0 if len(set(r)) == 3 else 2) | (4 if no_area(verts, r) else 0)
        key = tuple(sorted(r))
        if not bits & 2 and key in seen:
            bits |= 8
        seen.add(key)                                           # (every present face of a lower index, whatever became of it)
        out.append(bits)
    return out


def drop(verts, faces):
    return [r for r, b in zip(rows_of(faces), drop_bits(verts, faces)) if b == 0]


# ---- 3. orient ------------------------------------------------------------------------------------------------------------------------------
def adjacency(faces, V, same, opposite):
    """adj[f] = [(g, rel)] in the order of f's half-edges"""
    rows = rows_of(faces)
    along = {}                                                  # directed edge -> the counted faces that run along it
    for f, r in enumerate(rows):
        if counted(r, V):
            for k in range(3):
                along.setdefault((r[k], r[(k + 1) % 3]), []).append(f)
    adj = [[] for _ in rows]
    for f, r in enumerate(rows):
        if not counted(r, V):
            continue
        for k in range(3):
            s, o = same[3 * f + k], opposite[3 * f + k]
            if s + o != 2:
                continue
            u, w = r[k], r[(k + 1) % 3]
            others = [g for g in (along[(u, w)] if s == 2 else along[(w, u)]) if g != f]
            adj[f].append((others[0], 1 if s == 2 else 0))
    return adj


def orient_labels(faces, V, same, opposite):
    """(labels at the fixed point, rounds up to and including the first that changed nothing)"""
    adj = adjacency(faces, V, same, opposite)
    lab = [2 * f for f in range(len(adj))]
    for rounds in range(1, len(adj) + 9):
        new = [min([lab[f]] + [lab[g] ^ rel for g, rel in adj[f]]) for f in range(len(adj))]
        if new == lab:
            return lab, rounds
        lab = new
    raise AssertionError("no fixed point")


def orient_conflicts(faces, V, same, opposite, lab):
    adj = adjacency(faces, V, same, opposite)
    marks = [0] * len(adj)
    for f in range(len(adj)):
        for g, rel in adj[f]:
            if lab[f] >> 1 == lab[g] >> 1 and ((lab[f] ^ lab[g]) & 1) != rel:
                marks[lab[f] >> 1] = 1
    return marks


def orient_apply(faces, lab, nonorient, patch_flip=None):
    out = []
    for f, r in enumerate(rows_of(faces)):
        root = lab[f] >> 1
        swap = not nonorient[root] and ((lab[f] & 1) ^ (1 if patch_flip is not None and patch_flip[root] else 0))
        out.append((r[0], r[2], r[1]) if swap else r)
    return out


def patch_volumes(verts, faces, lab, same, opposite):
    """{root: six times the signed volume} of the patches without an open edge, summed in float64 in face order"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    open_roots, vol = set(), {}
    for f, r in enumerate(rows_of(faces)):
        root = lab[f] >> 1
        if any(same[3 * f + k] + opposite[3 * f + k] == 1 for k in range(3)):
            open_roots.add(root)
        a, b, c = (tuple(float(x) for x in v[i]) for i in r)
        t = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0])
        vol[root] = vol.get(root, 0.0) + t
    return {root: x for root, x in vol.items() if root not in open_roots}


def orient(verts, faces):
    """(faces, {"rounds", "non_orientable", "flipped_patches"}) on faces that are all counted"""
    V = np.asarray(verts).shape[0]
    same, opposite, _ = R.census(faces, V)
    lab, rounds = orient_labels(faces, V, same, opposite)
    marks = orient_conflicts(faces, V, same, opposite, lab)
    out = orient_apply(faces, lab, marks)
    even = [x & ~1 for x in lab]
    flip = [0] * len(lab)
    for root, x in patch_volumes(verts, out, lab, same, opposite).items():
        if x < 0 and not marks[root]:
            flip[root] = 1
    if any(flip):
        out = orient_apply(out, even, marks, flip)
    return out, {"rounds": rounds, "non_orientable": sum(marks), "flipped_patches": sum(flip)}


# ---- 4. cut ---------------------------------------------------------------------------------------------------------------------------------
def vertex_open(faces, V, same, opposite, flags):
    """(bad [V], next [V])"""
    out = [[] for _ in range(V)]
    for f, r in enumerate(rows_of(faces)):                       # ascending corner: the order of u's list
        for k in range(3):
            if same[3 * f + k] == 1 and opposite[3 * f + k] == 0:
                out[r[k]].append(r[(k + 1) % 3])
    bad = [1 if (flags[u] & WINDING_BITS) or len(out[u]) >= 2 else 0 for u in range(V)]
    return bad, [out[u][0] if len(out[u]) == 1 else -1 for u in range(V)]


def trouble(faces, V, per_face, bad):
    return [1 if present(r, V) and (per_face[f] > 0 or any(bad[i] for i in r)) else 0 for f, r in enumerate(rows_of(faces))]


def grow(faces, V, marks):
    rows = rows_of(faces)
    touched = {i for r, t in zip(rows, marks) if t and present(r, V) for i in r}
    return [1 if t or (present(r, V) and any(i in touched for i in r)) else 0 for r, t in zip(rows, marks)]


# ---- 5. fill --------------------------------------------------------------------------------------------------------------------------------
def loop_labels(bad, nxt):
    """(labels, jump) after DOUBLING_ROUNDS rounds"""
    V = len(nxt)
    lab, jump = list(range(V)), [-1 if bad[v] else nxt[v] for v in range(V)]
    for _ in range(DOUBLING_ROUNDS):
        lab, jump = ([min(lab[v], lab[jump[v]]) if 0 <= jump[v] < V else lab[v] for v in range(V)],
                     [jump[jump[v]] if 0 <= jump[v] < V else -1 for v in range(V)])
    return lab, jump


def loop_flags(bad, nxt, lab, jump, max_hole_edges):
    """(state [V], length [V], members {x: ascending vertices})"""
    V = len(nxt)
    members = {}
    for v in range(V):
        if 0 <= jump[v] < V:
            members.setdefault(lab[v], []).append(v)
    state, length = [0] * V, [0] * V
    for x in range(V):
        if not (0 <= jump[x] < V) or lab[x] != x:
            continue
        n = length[x] = len(members[x])
        state[x] = 2
        if 3 <= n <= max_hole_edges:
            u, steps = nxt[x], 1
            while steps < n and 0 <= u < V and u != x and not bad[u] and lab[u] == x:
                u, steps = nxt[u], steps + 1
            if u == x and steps == n:
                state[x] = 1
    return state, length, members


def mean32(rows, idx):
    """the float64 sum in the order of idx, divided once, rounded once to float32"""
    out = []
    for k in range(3):
        s = 0.0
        for i in idx:
            s += float(rows[i][k])
        out.append(np.float32(s / float(len(idx))))
    return out


def fill_emit(verts, colors, nxt, state, length, members):
    """(new faces, new verts [n, 3] float32, new colours or None)"""
    v = np.asarray(verts, dtype=np.float32)
    V = v.shape[0]
    faces, nv, nc = [], [], []
    for x in range(V):
        if state[x] != 1:
            continue
        if length[x] == 3:
            n1 = nxt[x]
            faces.append((nxt[n1], n1, x))
            continue
        m = V + len(nv)
        nv.append(mean32(v, members[x]))
        if colors is not None:
            nc.append(mean32(np.asarray(colors, dtype=np.float32), members[x]))
        faces += [(nxt[u], u, m) for u in members[x]]
    return (faces, np.asarray(nv, dtype=np.float32).reshape(-1, 3),
            np.asarray(nc, dtype=np.float32).reshape(-1, 3) if colors is not None else None)


# ---- 6. the loop ----------------------------------------------------------------------------------------------------------------------------
def _check(verts, faces):
    """what one check of the loop reads: per_face, the census, and the margin it was decided with"""
    V = np.asarray(verts).shape[0]
    hits = R.pair_rule(torch.from_numpy(np.asarray(verts, dtype=np.float32)), torch.tensor(faces, dtype=torch.long).reshape(-1, 3))
    return R.degrees(hits["pairs"], len(faces)), len(hits["pairs"]), R.census(faces, V), hits["margin"]


def report(verts, faces):
    return R.report(torch.from_numpy(np.ascontiguousarray(np.asarray(verts, dtype=np.float32))), torch.tensor(faces, dtype=torch.long).reshape(-1, 3))


def compact_vertices(verts, faces, colors):
    v = np.asarray(verts, dtype=np.float32)
    used = sorted({i for r in faces for i in r})
    new = {i: n for n, i in enumerate(used)}
    return v[used], [tuple(new[i] for i in r) for r in faces], (np.asarray(colors, dtype=np.float32)[used] if colors is not None else None)


def repair(verts, faces, colors=None, grow_times=1, max_rounds=8, max_hole_edges=None, do_orient=True, do_weld=True):
    """{"verts", "faces", "colors", "history", "stopped", "orient", "loops_left", "margins"}: repair_mesh restated"""
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.float32)).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(np.asarray(colors, dtype=np.float32)).reshape(-1, 3)
    f = rows_of(faces)
    cap = 2 ** 31 - 1 if max_hole_edges is None else max_hole_edges
    f0 = list(f)
    if do_weld:
        f = remap_faces(f, weld(v))
    f = drop(v, f)
    if not f:
        raise ValueError("nothing is left of the mesh")
    info = {"rounds": 0, "non_orientable": 0, "flipped_patches": 0}
    if do_orient:
        f, info = orient(v, f)
    history, margins, stopped, left = [], [], "max_rounds", 0
    for _ in range(max_rounds):
        V = v.shape[0]
        per_face, pairs, (same, opposite, flags), margin = _check(v, f)
        margins.append(margin)
        bad, nxt = vertex_open(f, V, same, opposite, flags)
        marks = trouble(f, V, per_face, bad)
        cut = 0
        g = f
        if any(marks):
            for _ in range(grow_times):
                marks = grow(f, V, marks)
            g = [r for r, t in zip(f, marks) if not t]
            cut = len(f) - len(g)
        if not g:
            stopped = "empty"
            break
        bad2, nxt2 = bad, nxt
        if cut:
            s2, o2, fl2 = R.census(g, V)
            bad2, nxt2 = vertex_open(g, V, s2, o2, fl2)
        lab, jump = loop_labels(bad2, nxt2)
        state, length, members = loop_flags(bad2, nxt2, lab, jump, cap)
        filled, left = state.count(1), state.count(2)
        if cut == 0 and filled == 0:
            stopped = "clean"
            break
        new_faces, new_verts, new_colors = fill_emit(v, c, nxt2, state, length, members)
        v2 = np.concatenate([v, new_verts]) if len(new_verts) else v
        c2 = np.concatenate([c, new_colors]) if c is not None and len(new_verts) else c
        h = drop(v2, g + new_faces)
        if not h:
            stopped = "empty"
            break
        if cut == 0 and h == f:                                 # every new face was a duplicate (a lone triangle's loop): the round undid itself
            stopped = "stalled"
            break
        if do_orient and any(x & R.WINDING for x in R.census(h, v2.shape[0])[2]):
            h, _ = orient(v2, h)
        history.append({"faces": len(f), "pairs": pairs, "bad_vertices": sum(bad), "open_edges": sum(1 for s, o in zip(same, opposite) if s == 1 and o == 0),
                        "faces_cut": cut, "loops_filled": filled, "loops_left": left, "vertices_added": int(len(new_verts)),
                        "faces_filled": len(new_faces), "faces_dropped": len(g) + len(new_faces) - len(h), "faces_after": len(h)})
        v, c, f = v2, c2, h
    untouched = stopped == "clean" and not history and f == f0
    if not untouched:
        v, f, c = compact_vertices(v, f, c)
    after = report(v, f)
    margins.append(R.pair_rule(torch.from_numpy(v), torch.tensor(f, dtype=torch.long).reshape(-1, 3))["margin"])
    return {"verts": v, "faces": f, "colors": c, "history": history, "stopped": stopped, "orient": info, "loops_left": left, "margins": margins,
            "after": after}


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------
def icosphere():
    v, f = R.census_mesh("icosphere")
    return v.numpy().copy(), rows_of(f)


def star_removed(vertex):
    v, f = icosphere()
    return v, [r for r in f if vertex not in r]


def faces_removed(a, b):
    v, f = icosphere()
    return v, [r for i, r in enumerate(f) if i not in (a, b)]


def soup(verts, faces):
    """every face with its own three vertices"""
    v = np.asarray(verts, dtype=np.float32)
    rows = rows_of(faces)
    return np.concatenate([v[list(r)] for r in rows]), [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(len(rows))]


def randomly_flipped(share=0.3, seed=5):
    v, f = icosphere()
    g = torch.Generator().manual_seed(seed)
    pick = torch.rand(len(f), generator=g) < share
    pick[0] = False                                             # (face 0 is the root: it keeps the patch's winding)
    return v, [(r[0], r[2], r[1]) if bool(p) else r for r, p in zip(f, pick)]


def inside_out():
    v, f = icosphere()
    return v, [(r[0], r[2], r[1]) for r in f]


def moebius(n=12):
    """a strip of n quads with a half twist: one side, one boundary loop of 2 n edges"""
    v, f = [], []
    for i in range(n):
        a = 2 * math.pi * i / n
        for s in (-0.3, 0.3):
            r = 1.0 + s * math.cos(a / 2)
            v.append((r * math.cos(a), r * math.sin(a), s * math.sin(a / 2)))
    for i in range(n):
        p0, p1 = 2 * i, 2 * i + 1
        q0, q1 = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < n else (1, 0)
        f += [(p0, q0, q1), (p0, q1, p1)]
    return np.asarray(v, dtype=np.float32), f


def named(name):
    """(verts float32 numpy, faces as rows) of a whole-loop scene"""
    kind, _, arg = name.partition("-")
    if kind == "fold":
        v, f = R.scene(name)
        return v.numpy().copy(), rows_of(f)
    if kind == "pair":
        v, f = R.scene(name)
        return v.numpy().copy(), rows_of(f)
    if kind == "single":
        v, f = R.scene(name)
        return v.numpy().copy(), rows_of(f)
    if kind == "star":
        return star_removed(int(arg))
    if kind == "two":
        return faces_removed(*(int(x) for x in arg.split("_")))
    if kind in R.CENSUS_MESHES:
        v, f = R.census_mesh(kind)
        return v.numpy().copy(), rows_of(f)
    table = {"soup": lambda: soup(*icosphere()), "mixed": randomly_flipped, "inside_out": inside_out, "moebius": moebius,
             "flipped_soup": lambda: soup(*named("flipped"))}
    return table[kind]()


# whole-loop scenes that keep SCENE_MARGIN in every round: (name, keyword arguments of repair)
MARGIN_SCENES = tuple((f"fold-{s}", {"grow_times": g}) for s in R.SEEDS for g in (1, 2)) + tuple((f"star-{x}", {}) for x in (12, 29, 72, 100, 150)) \
    + tuple((f"two-{a}_{b}", {}) for a, b in ((0, 1), (37, 36), (74, 69), (148, 24)))
# scenes decided by integers alone, or whose margin is not at stake
PLAIN_SCENES = tuple((n, {}) for n in ("soup", "mixed", "inside_out", "flipped_soup", "fin", "bow_tie", "cases", "icosphere")) \
    + (("open_grid", {"max_hole_edges": 8}),)
# scenes that do not keep the margin: only the weaker statements hold of them.  (open_grid without a cap is fanned shut from one centre in its
# own plane, so the second round's pair rule stands at margin 0;  the Moebius strip is all but flat where its cap crosses it.)
WEAK_SCENES = (("pair-1", {}), ("fold-1", {"grow_times": 0}), ("open_grid", {}), ("moebius", {}))


def key_of(name, kw):
    return name + "".join(f"[{k}={x}]" for k, x in sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _restated(name, items):
    v, f = named(name)
    grey = np.linspace(0.1, 0.9, 3 * v.shape[0], dtype=np.float32).reshape(-1, 3)
    return repair(v, f, grey, **dict(items))


def restated(name, kw):
    """repair() of a scene with a colour ramp, computed once"""
    return _restated(name, tuple(sorted(kw.items())))


def scene_colors(V):
    return np.linspace(0.1, 0.9, 3 * V, dtype=np.float32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _stages(name, items):
    kw = dict(items)
    v, f = named(name)
    V = v.shape[0]
    c = scene_colors(V)
    out = {"verts": v, "colors": c, "faces": f, "remap": weld(v)}
    out["faces_welded"] = remap_faces(f, out["remap"])
    out["drop"] = drop_bits(v, out["faces_welded"])
    fo = out["faces_kept"] = drop(v, out["faces_welded"])
    same, opposite, _ = R.census(fo, V)
    out["orient_same"], out["orient_opposite"] = same, opposite
    out["labels"], out["orient_rounds"] = orient_labels(fo, V, same, opposite)
    out["nonorient"] = orient_conflicts(fo, V, same, opposite, out["labels"])
    out["faces_applied"] = orient_apply(fo, out["labels"], out["nonorient"])
    fc, _ = orient(v, fo)
    out["faces_oriented"] = fc
    per_face, _, (same, opposite, flags), _ = _check(v, fc)
    out["per_face"], out["same"], out["opposite"], out["flags"] = per_face, same, opposite, flags
    out["bad"], out["next"] = vertex_open(fc, V, same, opposite, flags)
    marks = out["trouble"] = trouble(fc, V, per_face, out["bad"])
    if any(marks):
        for _ in range(kw.get("grow_times", 1)):
            marks = grow(fc, V, marks)
    out["grown"] = marks
    g = out["faces_cut"] = [r for r, t in zip(fc, marks) if not t]
    if not g:
        return out
    s2, o2, fl2 = R.census(g, V)
    out["cut_same"], out["cut_opposite"], out["cut_flags"] = s2, o2, fl2
    out["cut_bad"], out["cut_next"] = vertex_open(g, V, s2, o2, fl2)
    out["loop_labels"], out["loop_jump"] = loop_labels(out["cut_bad"], out["cut_next"])
    cap = kw.get("max_hole_edges") or 2 ** 31 - 1
    out["state"], out["length"], members = loop_flags(out["cut_bad"], out["cut_next"], out["loop_labels"], out["loop_jump"], cap)
    out["cap"] = cap
    out["new_faces"], out["new_verts"], out["new_colors"] = fill_emit(v, c, out["cut_next"], out["state"], out["length"], members)
    return out


def stages(name, kw):
    """what every pass reads and writes in the first round of repair() on a scene: the inputs and wanted outputs of the raw entries"""
    return _stages(name, tuple(sorted(kw.items())))
