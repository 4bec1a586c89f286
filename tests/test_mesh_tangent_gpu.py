"""The gfx950 tangent-space kernels and the GLB export (csrc_recon/meshtangent.hip, v3d_amd/recon/mesh_gltf.py, scripts/pub/export_glb.py)
against the torch restatement (tests/mesh_tangent_ref.py): corner frames, encode and decode with their round trip and a rigid motion, guards
around every output, the lit shade, the whole chain on the project's own extracted and decimated mesh through a written GLB, the script, and
the empty cases.

The bar everywhere is that of tests/test_mesh_texture_gpu.py: the kernel may be off from the fp64 restatement by 4x what the restatement's
own float32 run is off, the float32 figure taken once over the whole case (a prefix of the sphere's faces is held to the sphere's figure).  An
element is left out only when a length or |det| lies within a factor 2 of its threshold; tests/test_mesh_tangent_cpu.py holds every case to
0 % left out on the restatement alone.  Every kernel is fed to its restatement with the kernel's own inputs (the frames the device
computed, the view the device rasterized): one stage is compared at a time."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_bake_ref as B
import mesh_render_ref as M
import mesh_tangent_ref as T
import mesh_texture_ref as TX
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_bake as MB
from v3d_amd.recon import mesh_clean as MC
from v3d_amd.recon import mesh_decimate as MD
from v3d_amd.recon import mesh_gltf as MG
from v3d_amd.recon import mesh_texture as MT

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
UP = torch.tensor([0.0, 0.0, 1.0])
GUARD = 4096


def _dev(t, dtype=None):
    return t.to(DEV, dtype).contiguous() if dtype else t.to(DEV).contiguous()


def guarded(n, dtype):
    fill = float("nan") if dtype == F32 else -7
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_hold(buf, n, what):
    b = buf.cpu()
    lo, mid, hi = b[:GUARD], b[GUARD:GUARD + n], b[GUARD + n:]
    if b.dtype == F32:
        assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()), f"{what}: a guard was written"
        assert not torch.isnan(mid).any(), f"{what}: an element was left unwritten"
    else:
        assert bool((lo == -7).all()) and bool((hi == -7).all()), f"{what}: a guard was written"
        assert not (mid == -7).any(), f"{what}: an element was left unwritten"


def ok(rc, what):
    G._check(G.load_library(), rc, what)


# ---- 1. corner frames -------------------------------------------------------------------------------------------------------------------------
def run_frames(v, f, n):
    """the entry itself, between guards: (cn [3F, 3], ct [3F, 4]) on the host"""
    lib = G.load_library()
    F = f.shape[0]
    vd, fd, nd = _dev(v, F32), _dev(f, torch.int32), _dev(n, F32)
    cn_b, cn = guarded(9 * F, F32)
    ct_b, ct = guarded(12 * F, F32)
    ok(lib.v3d_recon_tex_corner_frames(vd.data_ptr(), v.shape[0], fd.data_ptr(), F, nd.data_ptr(), cn.data_ptr(), ct.data_ptr(), None), "corner_frames")
    torch.cuda.synchronize()
    guards_hold(cn_b, 9 * F, "corner_normals")
    guards_hold(ct_b, 12 * F, "corner_tangents")
    return cn.cpu().reshape(-1, 3), ct.cpu().reshape(-1, 4)


@pytest.mark.parametrize("name", T.FRAME_CASES)
def test_corner_frames_match_the_restatement(name):
    v, f, n, scene = T.frame_case(name)
    r64, _ = T.frame_restatements(name)
    s64, s32 = T.frame_restatements(scene)
    cn, ct = run_frames(v, f, n)
    again = run_frames(v, f, n)
    assert torch.equal(cn, again[0]) and torch.equal(ct, again[1]), "two runs differ"
    assert bool((ct[:, 3] == -1).all())
    cn_err, ct_err = T.frame_errors(cn, ct, r64)
    cn32, ct32 = T.frame_errors(s32["cn"], s32["ct"], s64)
    print(f"{name}: {cn.shape[0]} corners; normals {cn_err:.3e} (float32 restatement {cn32:.3e}), tangents {ct_err:.3e} ({ct32:.3e})")
    record_parity(f"mesh_tangent_frames[{name}]", {"normal_max_abs": cn_err, "normal_float32_restatement": cn32, "tangent_max_abs": ct_err,
                                                   "tangent_float32_restatement": ct32, "corners": int(cn.shape[0]),
                                                   "excluded_share": 1 - float(r64["keep"].float().mean())})
    assert cn_err <= 4 * cn32 and ct_err <= 4 * ct32
    assert float((cn.norm(dim=1) - 1).abs().max()) < 1e-6 and float((ct[:, :3].norm(dim=1) - 1).abs().max()) < 1e-6
    if name == "degenerate":                           # the face with index V: the defaults, exactly; nothing was read through it
        assert cn[963:].tolist() == [[0, 0, 1]] * 3 and ct[963:].tolist() == [[1, 0, 0, -1]] * 3
    if name == "fallback":
        assert ct[0].tolist() == [1, 0, 0, -1] and ct[1].tolist() == [1, 0, 0, -1] and cn[:2].tolist() == [[0, 0, 1], [0, 0, -1]]
    # the public function: the same frames from the same normals, and the device's own vertex normals by default
    pub = MG.corner_frames(v, f[:320] if name == "degenerate" else f, normals=n)
    k = pub[0].shape[0]
    assert torch.equal(pub[0].cpu(), cn[:k]) and torch.equal(pub[1].cpu(), ct[:k])
    if name == "sphere":
        own = MG.corner_frames(v, f)
        assert float((own[0].cpu() - cn).abs().max()) < 1e-6 and float((own[1].cpu() - ct).abs().max()) < 1e-6


# ---- 2. encode and decode ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_low_mesh():
    lv, lf, _ = T.low_mesh()
    lvd, lfd = _dev(lv), _dev(lf, torch.int32)
    ln = MC.vertex_normals(lvd, lfd)
    cn, ct = MG.frames_on_device(lvd, lfd, ln)
    return lv, lf, lvd, lfd, ln, cn, ct


@functools.lru_cache(maxsize=None)
def object_map(source, tex):
    """the bumped sphere's normals baked onto the icosphere by the device ("baked"), or (0, 0, 1) everywhere ("constant"): [R*R, 3] on the device"""
    if source == "constant":
        return _dev(T.constant_map(tex))
    lv, lf, hv, hf, md = B.bake_scene("nested")
    return MB.bake_normal_map(lv, lf, hv, hf, tex_size=tex, max_dist=md)[0]


def run_convert(fd, V, cn, ct, src, tex, encode):
    """the entry itself, between guards: (owner [R*R], map [R*R, 3]) on the host"""
    lib = G.load_library()
    ow_b, ow = guarded(tex * tex, torch.int32)
    out_b, out = guarded(3 * tex * tex, F32)
    fn = lib.v3d_recon_tex_encode_tangent if encode else lib.v3d_recon_tex_decode_tangent
    ok(fn(fd.data_ptr(), fd.shape[0], V, cn.data_ptr(), ct.data_ptr(), src.data_ptr(), tex, ow.data_ptr(), out.data_ptr(), None), "convert")
    torch.cuda.synchronize()
    guards_hold(ow_b, tex * tex, "owner")
    guards_hold(out_b, 3 * tex * tex, "map")
    return ow.cpu().long(), out.cpu().reshape(-1, 3)


def map_error(got, ref, rows):
    return float((got.double() - ref.double())[rows].abs().max()) if bool(rows.any()) else 0.0


@pytest.mark.parametrize("source", ("baked", "constant"))
@pytest.mark.parametrize("tex", T.MAP_SIZES)
def test_encode_and_decode_match_the_restatement(tex, source):
    lv, lf, lvd, lfd, ln, cn, ct = device_low_mesh()
    V = lv.shape[0]
    m = object_map(source, tex)
    cnh, cth, mh = cn.cpu(), ct.cpu(), m.cpu()
    owner, tm = run_convert(lfd, V, cn, ct, m, tex, True)
    again = run_convert(lfd, V, cn, ct, m, tex, True)
    assert torch.equal(owner, again[0]) and torch.equal(tm, again[1]), "two runs differ"
    e64, e32 = (T.convert_map(lf, V, cnh, cth, mh, tex, True, dt) for dt in (F64, F32))
    live = e64["live"]
    assert torch.equal(owner, e64["owner"]) and torch.equal(owner, TX.texel_cells(320, tex)[0]) and bool((tm[~live] == UP).all())
    rows = live & e64["keep"]
    enc_err, enc32 = map_error(tm, e64["map"], rows), map_error(e32["map"], e64["map"], rows)
    assert float((tm[live].norm(dim=1) - 1).abs().max()) < 1e-6
    # decode, of the kernel's own tangent map
    tmd = _dev(tm)
    owner2, back = run_convert(lfd, V, cn, ct, tmd, tex, False)
    again = run_convert(lfd, V, cn, ct, tmd, tex, False)
    assert torch.equal(owner2, again[0]) and torch.equal(back, again[1]) and torch.equal(owner2, owner) and bool((back[~live] == UP).all())
    d64, d32 = (T.convert_map(lf, V, cnh, cth, tm, tex, False, dt) for dt in (F64, F32))
    rows_d = live & d64["keep"]
    dec_err, dec32 = map_error(back, d64["map"], rows_d), map_error(d32["map"], d64["map"], rows_d)
    # the round trip: decode(encode(m)) against m, the float32 restatement's own round trip as the format's cost
    t32 = T.convert_map(lf, V, cnh, cth, e32["map"].float(), tex, False, F32)["map"]
    both = rows & rows_d
    trip_err, trip32 = map_error(back, mh, both), map_error(t32, mh, both)
    # the mesh rotated: its frames (the device's, from the rotated vertices and normals) decode the UNROTATED tangent map to Q m
    rv, rn = _dev(T.rotated(lv)), _dev(T.rotated(ln.cpu()))
    qcn, qct = MG.frames_on_device(rv, lfd, rn)
    _, moved = run_convert(lfd, V, qcn, qct, tmd, tex, False)
    q64 = T.corner_frames(rv.cpu(), lf, rn.cpu())
    want = T.convert_map(lf, V, q64["cn"], q64["ct"], e64["map"], tex, False)          # fp64 all the way from the rotated float32 mesh
    q32 = T.corner_frames(rv.cpu(), lf, rn.cpu(), F32)
    m32 = T.convert_map(lf, V, q32["cn"], q32["ct"], e32["map"], tex, False, F32)["map"]
    rows_q = both & want["keep"]
    rot_err, rot32 = map_error(moved, want["map"], rows_q), map_error(m32, want["map"], rows_q)
    rotated_m = torch.nn.functional.normalize(mh.double(), dim=1) @ T.rotation().t()
    physical = map_error(moved, rotated_m, rows_q)
    left_out = 1 - float(rows_q[live].float().mean())
    print(f"{source} R {tex}: {int(live.sum())} owned texels, {100 * left_out:.3f} % left out; encode {enc_err:.3e} (float32 restatement {enc32:.3e}), decode "
          f"{dec_err:.3e} ({dec32:.3e}), round trip {trip_err:.3e} ({trip32:.3e}), rotated {rot_err:.3e} ({rot32:.3e}), rotated against Q m {physical:.3e}")
    record_parity(f"mesh_tangent_maps[{source}-{tex}]", {"encode_max_abs": enc_err, "encode_float32_restatement": enc32, "decode_max_abs": dec_err,
                                                         "decode_float32_restatement": dec32, "round_trip_max_abs": trip_err,
                                                         "round_trip_float32_restatement": trip32, "rotated_max_abs": rot_err,
                                                         "rotated_float32_restatement": rot32, "rotated_against_Qm": physical, "excluded_share": left_out,
                                                         "owned": int(live.sum())})
    assert left_out <= T.EXCLUDE_MAX
    assert enc_err <= 4 * enc32 and dec_err <= 4 * dec32 and trip_err <= 4 * trip32 and rot_err <= 4 * rot32
    # Q m itself: the rotated mesh is rounded to float32 (6e-8 of a coordinate of 0.5) and so are the frames; 4 x what the float32 chain loses
    assert physical <= 4 * map_error(m32, rotated_m, rows_q)
    # the public functions: the same maps
    assert torch.equal(MG.to_tangent_space(lv, lf, m, tex, normals=ln).cpu(), tm) and torch.equal(MG.to_object_space(lv, lf, tm, tex, normals=ln).cpu(), back)
    assert torch.equal(MG.to_object_space(rv, lf, tm, tex, normals=rn).cpu(), moved)


def test_convert_writes_the_default_on_faces_outside_the_vertices():
    """the sphere plus a zero-area face and a face with index V, R = 100: the texels of the last face hold (0, 0, 1) both ways"""
    v, f, n, _ = T.frame_case("degenerate")
    vd, fd, nd = _dev(v), _dev(f, torch.int32), _dev(n)
    cn, ct = MG.frames_on_device(vd, fd, nd)
    m = _dev(T.random_maps(100)[1])
    for encode in (True, False):
        owner, out = run_convert(fd, v.shape[0], cn, ct, m, 100, encode)
        r = T.convert_map(f, v.shape[0], cn.cpu(), ct.cpu(), m.cpu(), 100, encode)
        assert torch.equal(owner, r["owner"]) and int((owner == 321).sum()) > 0 and bool((out[owner == 321] == UP).all()) and bool((out[owner < 0] == UP).all())
        rows = r["live"] & r["keep"]
        r32 = T.convert_map(f, v.shape[0], cn.cpu(), ct.cpu(), m.cpu(), 100, encode, F32)
        assert map_error(out, r["map"], rows) <= 4 * map_error(r32["map"], r["map"], rows)
        assert 1 - float(rows[r["live"]].float().mean()) <= T.EXCLUDE_MAX


# ---- 3. the lit shade -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lit_view(view):
    v, f, _ = M.mesh_scene(view[0], view[1])
    return v, f, MG.prepare_lit_view(M.case_camera(view), v, f, T.LIT_R, T.LIT_BG, cull=view[5])


@pytest.mark.parametrize("maps", ("both", "tangent", "ao", "none"))
@pytest.mark.parametrize("K", T.LIT_K)
@pytest.mark.parametrize("view", T.LIT_VIEWS, ids=M.case_id)
def test_shade_lit_matches_the_restatement(view, K, maps):
    v, f, lit = lit_view(view)
    W, H = view[2], view[3]
    albedo, tm, ao = T.random_maps(T.LIT_R)
    tm = tm if maps in ("both", "tangent") else None
    ao = ao if maps in ("both", "ao") else None
    lib = G.load_library()
    vw = lit.view
    # the view is mesh_texture's, bit for bit
    tv = MT.prepare_texture_view(M.case_camera(view), v, f, T.LIT_R, T.LIT_BG, cull=view[5], lists=False)
    assert torch.equal(tv.face_id, vw.face_id) and torch.equal(tv.pix_tex, vw.pix_tex) and torch.equal(tv.pix_tw, vw.pix_tw)
    dirs, inten = T.light_arrays(K)
    da = np.ascontiguousarray(np.stack(dirs) if K else np.zeros((0, 3)), dtype=np.float32)
    ia = np.ascontiguousarray(inten, dtype=np.float32)
    img_b, img = guarded(3 * H * W, F32)
    nrm_b, nrm = guarded(3 * H * W, F32)
    ald, tmd, aod = _dev(albedo), (_dev(tm) if tm is not None else None), (_dev(ao) if ao is not None else None)

    def run():
        ok(lib.v3d_recon_tex_shade_lit(vw.face_id.data_ptr(), lit.pix_w.data_ptr(), vw.pix_tex.data_ptr(), vw.pix_tw.data_ptr(), f.shape[0],
                                       lit.corner_normals.data_ptr(), lit.corner_tangents.data_ptr(), tmd.data_ptr() if tmd is not None else None,
                                       ald.data_ptr(), aod.data_ptr() if aod is not None else None, T.LIT_R, W, H, K, da.ctypes.data if K else None,
                                       ia.ctypes.data if K else None, T.LIT_AMBIENT, *T.LIT_BG, img.data_ptr(), nrm.data_ptr(), None), "shade_lit")
        torch.cuda.synchronize()
        guards_hold(img_b, 3 * H * W, "image")
        guards_hold(nrm_b, 3 * H * W, "normals")
        return img.cpu().reshape(3, H, W).clone(), nrm.cpu().reshape(3, H, W).clone()

    image, normals = run()
    again = run()
    assert torch.equal(image, again[0]) and torch.equal(normals, again[1]), "two runs differ"
    args = (vw.face_id.cpu(), lit.pix_w.cpu(), vw.pix_tex.cpu(), vw.pix_tw.cpu(), f.shape[0], lit.corner_normals.cpu(), lit.corner_tangents.cpu(), tm, albedo,
            ao, T.LIT_R, dirs, inten, T.LIT_AMBIENT, T.LIT_BG)
    r64, r32 = T.shade_lit(*args), T.shade_lit(*args, dtype=F32)
    cov = r64["covered"]
    assert torch.equal(cov, vw.face_id.cpu() >= 0) and 0.1 < float(cov.float().mean()) < 0.9
    assert bool((image[:, ~cov] == torch.tensor(T.LIT_BG)[:, None]).all()) and not normals[:, ~cov].any()          # exactly bg and 0 0 0
    rows = cov & r64["keep"]
    err = lambda a, k: float((a.double() - r64[k])[:, rows].abs().max())  # noqa: E731
    ierr, ierr32, nerr, nerr32 = err(image, "image"), err(r32["image"], "image"), err(normals, "normals"), err(r32["normals"], "normals")
    left_out = 1 - float(rows[cov].float().mean())
    print(f"{M.case_id(view)} K {K} {maps}: {int(cov.sum())} covered pixels, {100 * left_out:.3f} % left out; image {ierr:.3e} (float32 restatement {ierr32:.3e}), "
          f"normals {nerr:.3e} ({nerr32:.3e})")
    record_parity(f"mesh_tangent_lit[{M.case_id(view)}-K{K}-{maps}]", {"image_max_abs": ierr, "image_float32_restatement": ierr32, "normal_max_abs": nerr,
                                                                       "normal_float32_restatement": nerr32, "covered": int(cov.sum()),
                                                                       "excluded_share": left_out})
    assert left_out <= T.EXCLUDE_MAX and ierr <= 4 * ierr32 and nerr <= 4 * nerr32
    assert float((normals.norm(dim=0)[cov] - 1).abs().max()) < 1e-6
    # the public function
    pimg, pnrm = MG.shade_lit(lit, albedo, tm, ao, T.lights(K), T.LIT_AMBIENT)
    assert torch.equal(pimg.cpu(), image) and torch.equal(pnrm.cpu(), normals)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    N = B.E2E["N"]
    ref = B.bumpy_volume()
    f32 = lambda t, *s: t.float().reshape(*s).contiguous().to(DEV)  # noqa: E731
    vol = G.TsdfVolume(N, ref["bound"], ref["trunc"], f32(ref["tsdf_sum"], N, N, N), f32(ref["weight"], N, N, N), f32(ref["rgb_sum"], 3, N, N, N),
                       f32(ref["rgb_weight"], N, N, N))
    vf, ff, _ = G.extract_mesh(vol)
    vd, fd, _, _ = MD.decimate_mesh(vf, ff, None, B.E2E["target_faces"])
    return (vf, ff), (vd, fd), B.e2e_cameras()


def test_tangent_map_end_to_end(scene, tmp_path):
    """The mean angle to the high mesh's normals through (a) the low mesh's vertex normals, (b) the object-space map, (c) the float
    tangent-space map, (d) the 8-bit tangent-space map read back from the written GLB.  (d) must be below (a) by at least half of what (b)
    achieves.  (c) may differ from (b) only by what the fp64 restatement's (c) differs from its (b) ON THE SAME MESHES, NORMALS AND MAP (the
    device's, copied to the host), plus 4 x what the restatement's float32 runs of (b) and (c) are off."""
    (vf, ff), (vd, fd), cams = scene
    R = B.E2E["tex_size"]
    assert 1300 < ff.shape[0] < 1600 and fd.shape[0] in (299, 300) and len(cams) == 4 and int(cams[0].width) == 64
    nm, _ = MB.bake_normal_map(vd, fd, vf, ff, tex_size=R)
    tm = MG.to_tangent_space(vd, fd, nm, R)
    assert torch.equal(tm, MG.to_tangent_space(vd, fd, nm, R)), "two calls with the same arguments differ"
    fid = MB.normal_map_fidelity(vd, fd, nm, vf, ff, cams)
    a, b = fid["angle_before_mean"], fid["angle_after_mean"]
    ft = MG.tangent_map_fidelity(vd, fd, tm, vf, ff, cams)
    c = ft["angle_after_mean"]
    assert ft["pixels"] == fid["pixels"] and abs(ft["angle_before_mean"] - a) < 1e-9 and min(ft["pixels"]) > 400
    # without a map: the interpolated corner normals, about the vertex normals' value (perspective-correct instead of screen-space weights)
    plain = MG.tangent_map_fidelity(vd, fd, None, vf, ff, cams)["angle_after_mean"]
    assert abs(plain - a) < 0.05 * a
    # (d): through the file
    _, texture = MT.bake_vertex_colors(fd, M.position_colors(vd.cpu()), R)
    cn, ct = MG.corner_frames(vd, fd)
    path = str(tmp_path / "mesh.glb")
    size = MG.save_glb(path, vd, fd, texture, tangent_map=tm, tex_size=R, corner_normals=cn, corner_tangents=ct)
    T.parse_glb(open(path, "rb").read())
    back = MG.read_glb(path)
    assert size == os.path.getsize(path) and np.array_equal(back["verts"], vd.cpu().numpy()[fd.cpu().numpy().reshape(-1)])
    assert np.array_equal(back["normals"], cn.cpu().numpy()) and np.array_equal(back["tangents"], ct.cpu().numpy())
    assert float(np.abs(back["tangent_map"] - tm.cpu().numpy()).max()) <= 1.0 / 255 + 1e-6
    d = MG.tangent_map_fidelity(vd, fd, back["tangent_map"], vf, ff, cams)["angle_after_mean"]
    # the restatement on the device's meshes, vertex normals and object-space map
    lv, lf, hv, hf = vd.cpu(), fd.cpu().long(), vf.cpu(), ff.cpu().long()
    ln, hn, om = MC.vertex_normals(vd, fd).cpu(), MC.vertex_normals(vf, ff).cpu(), nm.cpu()
    rest = {}
    for key, dt in (("64", F64), ("32", F32)):
        _, rest["b" + key] = B.fidelity(lv, lf, ln, om, hv, hf, hn, cams, dt)
        fr = T.corner_frames(lv, lf, ln, dt)
        rtm = T.convert_map(lf, lv.shape[0], fr["cn"], fr["ct"], om, R, True, dt)["map"]
        rest["c" + key] = T.fidelity_tangent(lv, lf, ln, rtm, hv, hf, hn, cams, dt)
    allowed = abs(rest["c64"] - rest["b64"]) + 4 * (abs(rest["c32"] - rest["c64"]) + abs(rest["b32"] - rest["b64"]))
    print(f"{ff.shape[0]} -> {fd.shape[0]} faces, R {R}: mean angle to the high mesh's normals: (a) vertex normals {a:.4f}, (b) object-space map {b:.4f}, "
          f"(c) tangent-space map {c:.4f}, (d) 8-bit tangent-space map from the GLB {d:.4f} degrees; restatement on the same inputs (b) {rest['b64']:.4f} "
          f"(float32 {rest['b32']:.4f}), (c) {rest['c64']:.4f} (float32 {rest['c32']:.4f}); |c - b| {abs(c - b):.2e} of {allowed:.2e} allowed; GLB {size} bytes")
    record_parity("mesh_tangent_e2e", {"angle_vertex_normals": a, "angle_object_map": b, "angle_tangent_map": c, "angle_tangent_map_8bit_glb": d,
                                       "restatement_object_map": rest["b64"], "restatement_tangent_map": rest["c64"],
                                       "restatement_object_map_float32": rest["b32"], "restatement_tangent_map_float32": rest["c32"],
                                       "c_minus_b": c - b, "allowed": allowed, "faces_high": int(ff.shape[0]), "faces_low": int(fd.shape[0]),
                                       "glb_bytes": int(size)})
    assert a - b > 2.0                                  # the bake's own test holds this; here it is the premise
    assert a - d >= 0.5 * (a - b)
    assert abs(c - b) <= allowed
    frames = MG.render_lit_orbit(vd, fd, texture, tm, None, 2, *B.E2E["orbit"], 64, True)
    assert frames.shape == (2, 64, 64, 3) and frames.dtype == np.uint8 and int((frames != 255).any(-1).sum()) > 800
    flat = MG.render_lit_orbit(vd, fd, texture, None, None, 2, *B.E2E["orbit"], 64, True)
    assert int((frames != flat).any(-1).sum()) > 400          # the map is seen


def test_export_glb_script_end_to_end(scene, tmp_path):
    (vf, ff), (vd, fd), _ = scene
    R = B.E2E["tex_size"]
    low, high, obj = str(tmp_path / "low.ply"), str(tmp_path / "high.ply"), str(tmp_path / "nm.obj")
    G.save_mesh_ply(low, vd, fd, M.position_colors(vd.cpu()))
    G.save_mesh_ply(high, vf, ff, M.position_colors(vf.cpu()))
    spec = importlib.util.spec_from_file_location("v3d_entry_bake_normals", os.path.join(ROOT, "scripts", "pub", "bake_normals.py"))
    bake = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bake)
    bake.main(["--mesh", low, "--high", high, "-o", obj, "--texture_resolution", str(R), "--views", "0"])
    glb = str(tmp_path / "nm.glb")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pub", "export_glb.py"), "--mesh", obj, "-o", glb, "--render_orbit", "2", "--reso", "64",
                        "--elevation", "15", "-w", "--json", str(tmp_path / "nm_glb.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    size = os.path.getsize(glb)
    assert f"{fd.shape[0]} triangles" in r.stdout and f"{size} bytes" in r.stdout and "albedo, normal (tangent space)" in r.stdout and "occlusion" not in r.stdout
    assert sorted(os.listdir(tmp_path / "nm_lit_orbit")) == ["000.png", "001.png", "orbit.npy"]
    stats = json.load(open(tmp_path / "nm_glb.json"))
    assert stats["faces"] == fd.shape[0] and stats["bytes"] == size and stats["maps"] == ["albedo", "normal (tangent space)"] and stats["normal_source"] == "8-bit map"
    g = T.parse_glb(open(glb, "rb").read())
    back = MG.read_glb(glb)
    rv, rf, rvt, _ = MT.read_textured_obj(obj)
    assert np.array_equal(back["verts"], rv[rf.reshape(-1)]) and np.array_equal(back["faces"], np.arange(3 * rf.shape[0]).reshape(-1, 3))
    assert np.array_equal(back["uv"], ((rvt.reshape(-1, 2).astype(np.float64) + 0.5) / R).astype(np.float32))
    png = g["json"]["bufferViews"][g["json"]["images"][0]["bufferView"]]
    assert g["bin"][png["byteOffset"]:png["byteOffset"] + png["byteLength"]] == open(tmp_path / "nm.png", "rb").read()          # the albedo, byte for byte
    cn, ct = MG.corner_frames(vd, fd)
    assert np.array_equal(back["normals"], cn.cpu().numpy()) and np.array_equal(back["tangents"], ct.cpu().numpy())
    # the map decodes back to the OBJ's object-space map within the two quantisations
    om = MG.to_object_space(vd, fd, torch.from_numpy(back["tangent_map"]), R).cpu()
    from PIL import Image
    src = torch.from_numpy(np.asarray(Image.open(tmp_path / "nm_normal.png")).reshape(-1, 3).astype(np.float32) / 255.0 * 2 - 1)
    owned = MT.bake_vertex_colors(fd, torch.zeros(vd.shape[0], 3), R)[0].cpu() >= 0
    cos = (torch.nn.functional.normalize(om, dim=1) * torch.nn.functional.normalize(src, dim=1)).sum(1)[owned]
    assert float(torch.rad2deg(torch.acos(cos.clamp(-1, 1))).max()) < 2.0
    # in process: --high re-bakes in float and reports the angles both ways; a PLY input has no normalTexture without --high
    spec = importlib.util.spec_from_file_location("v3d_entry_export_glb", os.path.join(ROOT, "scripts", "pub", "export_glb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--mesh", obj, "--high", high, "-o", str(tmp_path / "hi.glb"), "--views", "4", "--reso", "64", "--elevation", "15", "--json", str(tmp_path / "hi.json")])
    st = json.load(open(tmp_path / "hi.json"))
    assert st["normal_source"] == "float bake" and st["angle_vertex"] - st["angle_tangent"] >= 0.5 * (st["angle_vertex"] - st["angle_object"]) > 1.0
    mod.main(["--mesh", low, "-o", str(tmp_path / "ply.glb"), "--texture_resolution", str(R)])
    pj = T.parse_glb(open(tmp_path / "ply.glb", "rb").read())["json"]
    assert "normalTexture" not in pj["materials"][0] and "occlusionTexture" not in pj["materials"][0] and len(pj["images"]) == 1
    pb = MG.read_glb(str(tmp_path / "ply.glb"))
    assert np.array_equal(pb["verts"], back["verts"]) and pb["tangent_map"] is None and pb["tex_size"] == R
    # the empty low mesh
    G.save_mesh_ply(str(tmp_path / "empty.ply"), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3))
    mod.main(["--mesh", str(tmp_path / "empty.ply"), "-o", str(tmp_path / "empty.glb"), "--texture_resolution", "16"])
    assert MG.read_glb(str(tmp_path / "empty.glb"))["verts"].shape == (0, 3)


# ---- 5. empty cases ---------------------------------------------------------------------------------------------------------------------------
def test_an_empty_low_mesh_is_answered_without_a_launch():
    v, f, _ = M.mesh_scene("sphere", 1)
    cam = B.e2e_cameras()[0]
    for lv, lf in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)), (v, torch.zeros(0, 3, dtype=torch.int64))):
        cn, ct = MG.corner_frames(lv, lf)
        assert cn.device.type == "cuda" and tuple(cn.shape) == (0, 3) and tuple(ct.shape) == (0, 4)
        tm = MG.to_tangent_space(lv, lf, torch.rand(1024, 3), 32)
        assert tm.device.type == "cuda" and bool((tm.cpu() == UP).all())
        lit = MG.prepare_lit_view(cam, lv, lf, 32, [1.0, 1.0, 1.0])
        img, nrm = MG.shade_lit(lit, torch.rand(1024, 3))
        assert bool((img == 1).all()) and not nrm.any()
        frames = MG.render_lit_orbit(lv, lf, torch.rand(1024, 3), None, None, 1, 2.0, 0.0, 60.0, 16)
        assert frames.shape == (1, 16, 16, 3) and bool((frames == 255).all())
