"""The isotropic remeshing of libv3d_recon.so (csrc_recon/meshremesh.hip, v3d_amd/recon/mesh_remesh.py, scripts/pub/remesh_mesh.py) without a
GPU: header, ctypes table and exports agree, bad arguments are refused before any launch, the host API refuses what does not fit and answers
empty meshes without a launch, the script's options are pinned, and the restatement (tests/mesh_remesh_ref.py) is honest: the operations of
a round touch pairwise disjoint faces and vertices, closed meshes stay closed manifolds, a mesh that is even already comes back unchanged,
open edges stay bit for bit, nothing is written past a capacity, the five measures of evenness all improve, and the cases of the GPU tests
sit far from the thresholds that float32 could move."""
import importlib.util
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import mesh_decimate_ref as Dm
import mesh_remesh_ref as Rm
import mesh_render_ref as M
from conftest import record_parity
from v3d_amd.recon import mesh_remesh as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"v3d_recon_remesh_split_propose", "v3d_recon_remesh_split_apply", "v3d_recon_remesh_collapse_propose", "v3d_recon_remesh_collapse_apply",
           "v3d_recon_remesh_flip_propose", "v3d_recon_remesh_flip_apply", "v3d_recon_remesh_relax", "v3d_recon_remesh_project"}
CLOSED = {"edges_twice_opposite": True, "euler": 2, "duplicates": 0, "degenerate": 0}


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


# ---- library --------------------------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert ENTRIES <= declared and declared == set(geometry.SIGNATURES)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert "Mesh remeshing" in hdr and "THE EDGE (a, b) IS EDITABLE" in hdr
    src = open(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshremesh.hip")).read()
    body = src.split("namespace {")[1]
    assert "#pragma clang fp contract(off)" in src and "atomic" not in body.lower() and "__shared__" not in body
    assert not re.search(r"\b(int|float|double|unsigned)\s+\w+\[\d*\]", body)          # no local arrays
    assert hex(Rm.KEY_HASH).upper()[2:] in src.upper() and Rm.KEY_HASH % 2 == 1


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p, q = 0x1000, 0x2000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731
    big = (2 ** 31 - 1) // 3 + 1                                      # 3 F would pass INT32_MAX
    counts = (dict(F=0), dict(V=0), dict(F=-2), dict(V=-1), dict(F=big))

    def calls(fn, order, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in order])

    def refuses(name, call, pointers, counts=counts):
        for k in pointers:
            assert call(**{k: None}) == -1 and name in err() and "null" in err(), (name, k)
        for kw in counts:
            assert call(**kw) == -1 and name in err() and "positive" in err(), (name, kw)

    lists = ("verts", "V", "faces", "F", "ranges", "corners")
    base = dict(verts=p, V=8, faces=p, F=4, ranges=p, corners=p, keys=p, targets=p, stream=None)
    for name in ("split", "collapse"):
        entry = f"v3d_recon_remesh_{name}_propose"
        pr = calls(getattr(lib, entry), lists + ("L", "cap", "keys", "targets", "stream"), L=0.1, cap=24, **base)
        refuses(entry, pr, ("verts", "faces", "ranges", "corners", "keys", "targets"))
        for cap in (2, 0, -1, 1025):
            assert pr(cap=cap) == -1 and entry in err() and "max_valence" in err(), cap
        for L in (0.0, -1.0, float("nan"), float("inf")):
            assert pr(L=L) == -1 and entry in err() and "target_edge" in err(), L
    fp = calls(lib.v3d_recon_remesh_flip_propose, lists + ("boundary", "cap", "keys", "targets", "stream"), boundary=p, cap=24, **base)
    refuses("v3d_recon_remesh_flip_propose", fp, ("verts", "faces", "ranges", "corners", "boundary", "keys", "targets"))
    assert fp(cap=2) == -1 and "max_valence" in err()
    sa = calls(lib.v3d_recon_remesh_split_apply, ("verts", "colors", "V", "faces", "F", "ranges", "corners", "accept", "targets", "rank", "cin", "cout",
                                                  "flag", "stream"), colors=p, accept=p, rank=p, cin=p, cout=q, flag=p, **base)
    refuses("v3d_recon_remesh_split_apply", sa, ("verts", "colors", "faces", "ranges", "corners", "accept", "targets", "rank", "cin", "cout", "flag"))
    assert sa(cout=p) == -1 and "two buffers" in err()
    ca = calls(lib.v3d_recon_remesh_collapse_apply, ("faces", "F", "V", "ranges", "corners", "accept", "targets", "removed", "stream"), accept=p,
               removed=p, **base)
    refuses("v3d_recon_remesh_collapse_apply", ca, ("faces", "ranges", "corners", "accept", "targets", "removed"))
    fa = calls(lib.v3d_recon_remesh_flip_apply, ("faces", "F", "V", "ranges", "corners", "accept", "targets", "stream"), accept=p, **base)
    refuses("v3d_recon_remesh_flip_apply", fa, ("faces", "ranges", "corners", "accept", "targets"))
    rx = calls(lib.v3d_recon_remesh_relax, lists + ("boundary", "pinned", "lam", "out", "stream"), boundary=p, pinned=None, lam=0.5, out=q, **base)
    refuses("v3d_recon_remesh_relax", rx, ("verts", "faces", "ranges", "corners", "boundary", "out"))
    assert rx(out=p) == -1 and "two buffers" in err()
    for lam in (-0.1, 1.5, float("nan")):
        assert rx(lam=lam) == -1 and "lambda" in err(), lam
    pj = calls(lib.v3d_recon_remesh_project, ("face", "uv", "sv", "sc", "V", "sf", "F", "verts", "colors", "N", "stream"), face=p, uv=p, sv=p, sc=p, sf=p,
               verts=q, colors=q, N=8, V=8, F=4, stream=None)
    refuses("v3d_recon_remesh_project", pj, ("face", "uv", "sv", "sc", "sf", "verts", "colors"))
    for n in (0, -1):
        assert pj(N=n) == -1 and "positive" in err()
    assert pj(verts=p) == -1 and "two buffers" in err()


# ---- host API -------------------------------------------------------------------------------------------------------------------------------
def test_host_api_refuses_what_does_not_fit_and_answers_empties_without_a_launch():
    v, f = M.icosphere(0)
    c = M.position_colors(v)
    cpu = dict(device="cpu")
    for bad, match in ((dict(target_edge=0.1, target_faces=10), "not both"), (dict(target_edge=0.0), "target_edge"), (dict(target_edge=float("nan")), "target_edge"),
                       (dict(target_faces=0), "target_faces"), (dict(target_faces=-3), "target_faces"), (dict(iterations=-1), "iterations"),
                       (dict(relax=1.5), "relax"), (dict(relax=-0.1), "relax"), (dict(max_valence=2), "max_valence"), (dict(max_rounds=-1), "max_rounds")):
        with pytest.raises(ValueError, match=match):
            MR.remesh_mesh(v, f, c, **bad, **cpu)
    with pytest.raises(ValueError, match="outside the vertex array"):
        MR.remesh_mesh(v, f + 1, c, **cpu)
    with pytest.raises(ValueError, match="12 vertices, 11 colours"):
        MR.remesh_mesh(v, f, c[:-1], **cpu)
    none = torch.zeros(0, 3, dtype=torch.int64)
    for vv, ff, cc in ((v, none, c), (v[:0], none, c[:0]), (v, none, None)):
        ov, of, oc, st = MR.remesh_mesh(vv, ff, cc, target_edge=0.1, **cpu)
        assert torch.equal(ov, vv) and of.shape == (0, 3) and of.dtype == torch.int32 and (oc is None if cc is None else torch.equal(oc, cc))
        assert st["operations"] == {"split": [], "collapse": [], "flip": []} and st["faces_after"] == 0 and st["vertices_after"] == vv.shape[0]
        json.loads(json.dumps(st, allow_nan=False))
    lib_defaults = {k: p.default for k, p in inspect.signature(MR.remesh_mesh).parameters.items()}
    assert lib_defaults["iterations"] == 3 and lib_defaults["relax"] == 0.5 and lib_defaults["reproject"] is True and lib_defaults["max_valence"] == 24
    assert MR.default_edge(_area(v, f), 20) == pytest.approx(Rm.default_edge(v.numpy(), f.numpy()), rel=1e-12)
    assert MR.default_edge(_area(v, f), 80) == pytest.approx(Rm.default_edge(v.numpy(), f.numpy(), 80), rel=1e-12)
    v2, f2, _ = Dm.scene("ico2")
    mine, ref = MR.mesh_measures(v2, f2), Rm.measures(v2.numpy(), f2.numpy())
    assert set(mine) == set(Rm.MEASURES) and all(mine[k] == pytest.approx(ref[k], rel=1e-12) for k in mine)


def _area(v, f):
    p = v.double()
    return float(0.5 * torch.linalg.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]).norm(dim=1).sum())


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _disjoint():
    seen = {"rounds": 0, "ops": 0}

    def check(op, touched):
        items = list(touched.values())
        for i in range(len(items)):
            for j in range(i):
                assert not (items[i][0] & items[j][0]), f"{op}: two operations of a round write one face"
                assert not (items[i][1] & items[j][1]), f"{op}: two operations of a round touch one vertex"
        seen["rounds"] += 1
        seen["ops"] += len(items)
    return check, seen


@pytest.mark.parametrize("name", tuple(Rm.LOOP_CASES))
def test_rounds_touch_disjoint_sets_and_closed_meshes_stay_closed_and_every_measure_improves(name):
    v, f, c = Rm.decimated(name)
    check, seen = _disjoint()
    vo, fo, co, st = Rm.remesh(v, f, c, iterations=3, check=check)
    assert seen["ops"] == sum(sum(n) for n in st["ops"].values()) > 100 and seen["rounds"] == sum(sum(n) for n in st["rounds"].values())
    ro, fo2 = Rm.loop_run(name)[0], Rm.loop_run(name)[1]
    assert np.array_equal(fo, fo2) and np.array_equal(vo, ro)                                    # the check changes nothing
    assert Dm.manifold_report(f, v.shape[0]) == {**CLOSED, "used_vertices": v.shape[0]}
    assert Dm.manifold_report(fo, vo.shape[0]) == {**CLOSED, "used_vertices": vo.shape[0]}
    before, after = Rm.measures(v, f), Rm.measures(vo, fo)
    dist = Rm.Q.mesh_distance(torch.from_numpy(vo).float(), torch.from_numpy(fo), torch.from_numpy(v), torch.from_numpy(f))
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
    far = float(max(dist["a_to_b"]["max"], dist["b_to_a"]["max"])) / diag
    print(f"{name}: {f.shape[0]} -> {fo.shape[0]} faces, {st}; before {before}; after {after}; {far:.4f} of the diagonal from the input")
    record_parity(f"mesh_remesh_restatement[{name}]", {"faces_before": int(f.shape[0]), "faces_after": int(fo.shape[0]), "operations": st["ops"],
                                                       "rounds": st["rounds"], "before": before, "after": after, "distance_over_diagonal": far})
    assert all(Rm.improved(before, after).values()), Rm.improved(before, after)
    assert far < 0.05                              # (the surface is the input's: every vertex was put back on it)
    assert sum(st["rounds"][op][-1] for op in st["rounds"]) <= 3       # the last iteration finds next to nothing left to do
    f32 = Rm.loop_run(name, "float32")
    assert Dm.manifold_report(f32[1], f32[0].shape[0]) == {**CLOSED, "used_vertices": f32[0].shape[0]}
    assert all(Rm.improved(before, Rm.measures(f32[0], f32[1])).values())


def test_an_even_mesh_comes_back_unchanged():
    v, f, c = Dm.scene("ico3")
    vo, fo, co, st = Rm.remesh(v.numpy(), f.numpy(), c.numpy(), iterations=3)
    assert np.array_equal(fo, f.numpy()) and all(n == [0, 0, 0] for n in st["ops"].values())
    assert vo.shape == tuple(v.shape) and not np.array_equal(vo, v.numpy().astype(np.float64))          # (the vertices slid within the surface)
    assert float(np.abs(np.linalg.norm(vo, axis=1) - 0.5).max()) < 2e-3                                  # .. and stayed on the sphere's polyhedron


def _open_edges(v, f):
    """(the positions of the vertices on open edges, the open edges as pairs of positions), both as sets of bytes"""
    und, cnt, _ = Dm.R.undirected_counts(np.asarray(f, dtype=np.int64))
    edges = np.asarray(und)[np.asarray(cnt) == 1]
    p = np.asarray(v, dtype=np.float32)
    return {p[i].tobytes() for i in np.unique(edges)}, {frozenset((p[a].tobytes(), p[b].tobytes())) for a, b in edges.tolist()}


def test_open_edges_and_their_vertices_stay_bit_for_bit():
    v, f, c, L = Rm.case("grid")
    check, seen = _disjoint()
    vo, fo, co, st = Rm.remesh(v, f, c, L=L, iterations=1, dtype=np.float32, check=check)
    assert st["ops"]["split"][0] > 300 and fo.shape[0] > 1.5 * f.shape[0] and seen["ops"] > 300
    assert _open_edges(v, f) == _open_edges(vo.astype(np.float32), fo)
    rim = Dm.grid_rim().numpy()
    assert len(_open_edges(v, f)[0]) == int(rim.sum()) and np.array_equal(vo[:v.shape[0]][rim].astype(np.float32), v[rim])
    rep = Dm.manifold_report(fo, vo.shape[0])
    assert rep["duplicates"] == 0 and rep["degenerate"] == 0 and rep["euler"] == 1              # still one disc


def test_vertices_above_the_cap_never_propose_and_are_no_collapse_target():
    v, f, c, L = Rm.case("bipyramid")
    assert f.shape[0] == Dm.FAN and Dm.FAN // 2 == 350 > Rm.DEFAULT_MAX_VALENCE
    proposals = 0
    for L_ in (L, 8 * L, 0.05 * L):
        st = Rm.State(v, f, c, 8)
        star = st.stars()
        for keys, targets, _ in (Rm.split_propose(st, L_, star=star), Rm.collapse_propose(st, L_, star=star), Rm.flip_propose(st, star=star)):
            assert keys[0] == keys[1] == Rm.NO_KEY and targets[0] == targets[1] == -1
            proposals += sum(k != Rm.NO_KEY for k in keys)
        ck, ct, _ = Rm.collapse_propose(st, L_, star=star)
        assert not {0, 1} & set(ct)
        info = Rm.collapse_analyse(st, L_, star=star)
        assert info[0] is None and info[1] is None and all("valence" in info[x][apex]["why"] for x in range(2, 352) for apex in (0, 1))
    assert proposals > 700
    st = Rm.State(v, f, c, 8)
    assert sum(t >= 2 for t in Rm.collapse_propose(st, 8 * L)[1]) == 350                      # it is the cap alone that keeps the apexes


def test_a_capacity_one_vertex_short_sets_the_flag_and_writes_nothing_past_it():
    v, f, c, L = Rm.case("net400")
    st = Rm.State(v, f, c, Rm.SPARE)
    keys, targets, _ = Rm.split_propose(st, L)
    accept = Dm.select(st.faces, keys)
    n = sum(accept)
    assert n >= 4
    short = Rm.State(v, f, c, n - 1)
    Rm.split_apply(short, accept, targets)
    assert short.flag and short.V_live == short.Vcap == v.shape[0] + n - 1 and short.F_live == short.Fcap == f.shape[0] + 2 * (n - 1)
    assert len(short.P) == short.Vcap and len(short.faces) == short.Fcap and all(t is not None for t in short.faces)
    Rm.split_apply(st, accept, targets)
    assert not st.flag and st.V_live == v.shape[0] + n
    assert short.faces[:f.shape[0] + 2 * (n - 1)] != st.faces[:f.shape[0] + 2 * (n - 1)]        # the split of the last rank was dropped whole ..
    last = max(a for a, on in enumerate(accept) if on)
    assert [t for t in short.faces if last in t] == [t for t in Rm.State(v, f, c, 0).faces if t is not None and last in t]      # .. its faces untouched
    vo, fo, _, stats = Rm.remesh(v, f, c, L=L, iterations=1, spare=n - 1)
    ref = Rm.remesh(v, f, c, L=L, iterations=1)
    assert stats["reallocations"] >= 1 and Dm.manifold_report(fo, vo.shape[0]) == {**CLOSED, "used_vertices": vo.shape[0]}
    assert fo.shape[0] == ref[1].shape[0]


def test_keys_are_distinct_and_ordered_by_priority():
    for name, op in (("net400", "split"), ("net", "collapse"), ("ico3_200", "flip")):
        st, keys, targets, _ = Rm.proposals(name, op)
        real = [k for k in keys if k != Rm.NO_KEY]
        assert len(real) > 40 and len(set(real)) == len(real)
        for v_, (k, t) in enumerate(zip(keys, targets)):
            assert (k == Rm.NO_KEY) == (t == -1)
            if k != Rm.NO_KEY:
                assert k & 0xFFFFFFFF == (v_ * Rm.KEY_HASH) % 2 ** 32 and (k >> 32) < 0x7F800000            # finite and not negative
    ids = [(v_ * Rm.KEY_HASH) % 2 ** 32 for v_ in range(100000)]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("name", tuple(Rm.CASES))
def test_premises_of_the_gpu_cases(name):
    """Both precisions take every threshold decision alike, but for at most 2 % of the vertices"""
    v, f, c, L = Rm.case(name)
    for op in ("split", "collapse", "flip"):
        st, k64, t64, margin = Rm.proposals(name, op)
        _, k32, t32, m32 = Rm.proposals(name, op, np.float32)
        out = Rm.excluded(margin)
        assert sum(out) <= Rm.EXCLUDE_MAX * len(out) and sum(Rm.excluded(m32)) <= Rm.EXCLUDE_MAX * len(out), (name, op)
        assert [(a == Rm.NO_KEY) for a, o in zip(k64, out) if not o] == [(a == Rm.NO_KEY) for a, o in zip(k32, out) if not o], (name, op)
    want = {"net400": (100, 3, 40), "ico3_200": (50, 3, 20), "net": (10, 100, 40), "noisy": (100, 20, 40), "grid": (200, 0, 100), "flat": (20, 40, 100),
            "single": (0, 0, 0), "bad_indices": (100, 0, 0), "degenerate": (100, 0, 0)}.get(name)
    if want is not None:                       # the cases are not idle: each operation has work where the tests look for it
        got = tuple(sum(k != Rm.NO_KEY for k in Rm.proposals(name, op)[1]) for op in ("split", "collapse", "flip"))
        assert all(g >= w for g, w in zip(got, want)), (name, got)
        if name == "single":
            assert got == (0, 0, 0)


@pytest.mark.parametrize("name", Rm.PLANTED)
def test_with_its_length_rules_open_wide_the_collapse_proposes_where_decimation_does(name):
    """The two restatements against each other: nothing else holds the rule of one collapse to the rule of the other"""
    v, f, c = Dm.scene(name)
    cap = Rm.DEFAULT_MAX_VALENCE
    decim_keys, info = Rm.decimation_verdict(name, cap)
    st = Rm.State(v.numpy(), f.numpy(), c.numpy(), 0)
    keys, targets, _ = Rm.collapse_propose(st, Rm.OPEN_WIDE, cap)
    analysis = Rm.collapse_analyse(st, Rm.OPEN_WIDE, cap)
    assert not any({"long", "stretch"} & c_["why"] for cand in analysis if cand for c_ in cand.values())          # the premise: both rules are open
    Rm.assert_collapse_proposers_agree(name, decim_keys, keys, targets, cap)
    proposing = sum(k != Rm.NO_KEY for k in keys)
    print(f"{name}: {proposing} of {len(keys)} vertices propose in both")
    assert proposing == {"tetrahedron": 0, "octahedron": 6, "bipyramid": 350, "dart": 1, "grid": int((~Dm.grid_rim()).sum())}[name]


# ---- script and files -----------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_are_pinned():
    mod = _entry("remesh_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh.ply", "-o", "out/gs/mesh_even.ply"]))
    assert a == {"mesh": "out/gs/mesh.ply", "out": "out/gs/mesh_even.ply", "target_edge": None, "target_faces": None, "iterations": 3, "relax": 0.5,
                 "no_reproject": False, "max_valence": 24, "json": None, "white_background": False, "render_orbit": 0, "video": None, "num_frames": None,
                 "reso": None, "radius": 2.0, "elevation": 0.0, "fov": 60.0}
    b = vars(ap.parse_args(["--mesh", "in.ply", "-o", "out.ply", "--target_faces", "50000", "--iterations", "5", "--relax", "0.25", "--no_reproject",
                            "--json", "s.json", "--render_orbit", "36", "-w", "--video", "orbit.npy"]))
    assert b["target_faces"] == 50000 and b["iterations"] == 5 and b["relax"] == 0.25 and b["no_reproject"] and b["json"] == "s.json"
    assert b["render_orbit"] == 36 and b["white_background"] and b["video"] == "orbit.npy"
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov", "white_background"):
        assert a[k] == recon[k], k
    with pytest.raises(SystemExit):
        ap.parse_args(["-o", "c.ply"])                   # --mesh is required
    for bad in (["--target_edge", "0"], ["--target_edge", "-1"], ["--target_edge", "nan"], ["--target_edge", "inf"], ["--target_faces", "0"],
                ["--target_edge", "0.1", "--target_faces", "100"], ["--iterations", "-1"], ["--relax", "2"], ["--relax", "nan"], ["--max_valence", "2"],
                ["--render_orbit", "-1"], ["--reso", "0"], ["--reso", "5000"]):
        with pytest.raises(SystemExit):
            mod.main(["--mesh", "does/not/exist.ply", "-o", "c.ply", *bad])
    lib_defaults = {k: p.default for k, p in inspect.signature(MR.remesh_mesh).parameters.items()}          # the script's defaults are the library's
    assert all(a[k] == lib_defaults[k] for k in ("target_edge", "target_faces", "iterations", "relax", "max_valence"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert readme.index("decimate_mesh.py") < readme.index("remesh_mesh.py")


def test_script_writes_strict_json_and_a_ply_that_loads(tmp_path):
    """Without a GPU only a mesh without faces gets through (no launch): the files are written all the same."""
    from v3d_amd.recon import geometry as G
    v, f = M.icosphere(0)
    ply, out, js = str(tmp_path / "mesh.ply"), str(tmp_path / "even.ply"), str(tmp_path / "stats.json")
    G.save_mesh_ply(ply, v, f[:0], M.position_colors(v))
    _entry("remesh_mesh").main(["--mesh", ply, "-o", out, "--target_edge", "0.1", "--json", js], device="cpu")
    assert sorted(os.listdir(tmp_path)) == ["even.ply", "mesh.ply", "stats.json"]

    def strict(token):
        raise ValueError(f"{token} is not JSON")
    stats = json.loads(open(js).read(), parse_constant=strict)
    assert stats["faces_before"] == 0 == stats["faces_after"] and stats["vertices_after"] == 12 and stats["target_edge"] == pytest.approx(0.1)
    rv, rf, rc = G.read_mesh_ply(out)
    rv0, rf0, rc0 = G.read_mesh_ply(ply)
    assert np.array_equal(rv, rv0) and np.array_equal(rf, rf0) and np.array_equal(rc, rc0)
