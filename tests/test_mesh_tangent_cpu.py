"""Tangent space and GLB export (csrc_recon/meshtangent.hip, v3d_amd/recon/mesh_gltf.py, scripts/pub/export_glb.py) without a GPU: header,
ctypes table and exports agree, bad arguments are refused before any launch, the convention worked out by hand, w derived from its
definition, the restatement's round trip and rigid motion (tests/mesh_tangent_ref.py), the GLB writer against a parser written from the
specification, writer -> reader, the script's options, and the premises of the cases of tests/test_mesh_tangent_gpu.py on the
restatement alone."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_render_ref as M
import mesh_tangent_ref as T
import mesh_texture_ref as TX
from v3d_amd.recon import mesh_gltf as MG                                       # (without the feature: the import fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"v3d_recon_tex_corner_frames", "v3d_recon_tex_encode_tangent", "v3d_recon_tex_decode_tangent", "v3d_recon_tex_shade_lit"}
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


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
    assert int(re.search(r"#define V3D_RECON_ABI_VERSION (\d+)", hdr).group(1)) == 1
    assert "Tangent space and GLB" in hdr and "THE TANGENT FRAME" in hdr
    assert int(re.search(r"#define V3D_RECON_LIT_MAX_LIGHTS (\d+)", hdr).group(1)) == MG.MAX_LIGHTS == 4
    src = open(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshtangent.hip")).read()
    assert "atomic" not in src.replace("No atomics", "") and "__shared__" not in src


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731

    def calls(fn, names, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in names])

    cf = calls(lib.v3d_recon_tex_corner_frames, ("verts", "V", "faces", "F", "normals", "cn", "ct", "stream"),
               verts=p, V=162, faces=p, F=320, normals=p, cn=p, ct=p, stream=None)
    for k in ("verts", "faces", "normals", "cn", "ct"):
        assert cf(**{k: None}) == -1 and "v3d_recon_tex_corner_frames" in err() and "null" in err(), k
    assert cf(V=0) == -1 and "num_verts" in err()
    assert cf(F=0) == -1 and "num_faces 0" in err()
    assert cf(F=-1) == -1 and "num_faces" in err()
    assert cf(F=(2 ** 31 - 1) // 3 + 1) == -1 and "int32" in err()
    for fn, name, src, dst in ((lib.v3d_recon_tex_encode_tangent, "v3d_recon_tex_encode_tangent", "object_map", "tangent_map"),
                               (lib.v3d_recon_tex_decode_tangent, "v3d_recon_tex_decode_tangent", "tangent_map", "object_map")):
        cv = calls(fn, ("faces", "F", "V", "cn", "ct", src, "R", "owner", dst, "stream"),
                   **{"faces": p, "F": 320, "V": 162, "cn": p, "ct": p, src: p, "R": 64, "owner": p, dst: p, "stream": None})
        for k in ("faces", "cn", "ct", src, "owner", dst):
            assert cv(**{k: None}) == -1 and name in err() and "null" in err(), k
        assert cv(V=0) == -1 and "num_verts" in err()
        assert cv(F=0) == -1 and "num_faces" in err()
        assert cv(R=0) == -1 and "tex_size 0" in err()
        assert cv(R=4097) == -1 and "tex_size 4097" in err()
        assert cv(R=32) == -1 and "too small" in err()
    names = ("face_id", "pix_w", "pix_tex", "pix_tw", "F", "cn", "ct", "tmap", "albedo", "ao", "R", "W", "H", "K", "dirs", "inten", "ambient", "bg0", "bg1",
             "bg2", "image", "normals", "stream")
    sl = calls(lib.v3d_recon_tex_shade_lit, names, face_id=p, pix_w=p, pix_tex=p, pix_tw=p, F=320, cn=p, ct=p, tmap=p, albedo=p, ao=p, R=64, W=64, H=48,
               K=5, dirs=p, inten=p, ambient=0.2, bg0=1.0, bg1=1.0, bg2=1.0, image=p, normals=p, stream=None)          # (K = 5: refused at the latest there)
    for k in ("face_id", "pix_w", "pix_tex", "pix_tw", "cn", "ct", "albedo", "image", "normals"):
        assert sl(**{k: None}) == -1 and "v3d_recon_tex_shade_lit" in err() and "null" in err(), k
    assert sl(F=0) == -1 and "num_faces 0" in err()
    assert sl(R=0) == -1 and "tex_size 0" in err()
    assert sl(R=4097) == -1 and "tex_size 4097" in err()
    assert sl(R=32) == -1 and "too small" in err()
    assert sl(W=0) == -1 and "image 0 x 48" in err()
    assert sl(H=4097) == -1 and "image" in err()
    assert sl(K=5) == -1 and "num_lights 5" in err() and "0 .. 4" in err()
    assert sl(K=-1) == -1 and "num_lights -1" in err()
    assert sl(K=2, dirs=None) == -1 and "light" in err()
    assert sl(K=2, inten=None) == -1 and "light" in err()
    # NULL maps are arguments, not errors: with them the next refusal is reached
    assert sl(tmap=None, ao=None) == -1 and "num_lights 5" in err()


# ---- the convention ---------------------------------------------------------------------------------------------------------------------------
def quad():
    """A unit quad in the xy plane facing +z whose two faces are laid out so that atlas u runs along +x in both halves: half 0 has
    dP/du = +e1 / L with e1 = +x; half 1 has dP/du = -e1 / L, so its e1 = -x."""
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    return v, torch.tensor([[0, 1, 2], [3, 2, 1]])


def test_the_convention_on_a_flat_quad():
    """By hand.  N = (0, 0, 1) everywhere.  T = normalise(s e1) = (+1, 0, 0) in both halves (e1 = (+1, 0, 0) in half 0 and (-1, 0, 0) in half
    1, s = +1 and -1).  Atlas v (image row, glTF v) grows along dP/dv = s e2 / L = +y in both halves, so DECREASING v is -y, and glTF's
    bitangent w cross(N, T) = w (0, 1, 0) must be (0, -1, 0): w = -1.  The object normal m = (0.3, 0.4, 1) / |.| leans towards +x (along T:
    red above 0.5) and towards +y, which is INCREASING v: green below 0.5.  c = (m . T, m . B, m . N) = (0.3, -0.4, 1) / sqrt(1.25)."""
    v, f = quad()
    n = C.normals(v, f)
    assert torch.equal(n, torch.tensor([[0.0, 0.0, 1.0]], dtype=F64).expand(4, 3))
    fr = T.corner_frames(v, f, n)
    e1 = v[f[:, 1]] - v[f[:, 0]]
    assert e1.tolist() == [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]
    assert torch.equal(fr["ct"][:, :3], torch.tensor([[1.0, 0.0, 0.0]], dtype=F64).expand(6, 3))
    assert bool((fr["ct"][:, 3] == -1).all()) and bool((T.derived_w(v, f, fr["cn"], fr["ct"]) == -1).all())
    cnh, cth = MG.corner_frames_host(v, f)
    assert np.array_equal(cnh, fr["cn"].float().numpy()) and np.array_equal(cth, fr["ct"].float().numpy())
    # u along +x and v along +y in the atlas itself
    uv, P = TX.face_uvs(2, 16), v[f].double()
    for k in range(2):
        du, dv = uv[k, 1] - uv[k, 0], uv[k, 2] - uv[k, 0]
        assert float(du[1]) == 0 and float(dv[0]) == 0
        assert ((P[k, 1] - P[k, 0]) / du[0]).tolist() == [1 / 13, 0, 0] and ((P[k, 2] - P[k, 0]) / dv[1]).tolist() == [0, 1 / 13, 0]
    m = torch.tensor([[0.3, 0.4, 1.0]], dtype=F64)
    m = m / m.norm()
    want = torch.tensor([0.3, -0.4, 1.0], dtype=F64) / math.sqrt(1.25)
    for face in (0, 1):
        frame = T.frame_at(fr["cn"], fr["ct"], torch.tensor([face]), torch.tensor([[0.2, 0.5, 0.3]], dtype=F64))
        c, keep, det = T.encode(frame, m)
        assert bool(keep.all()) and float((c[0] - want).abs().max()) < 1e-15 and abs(float(det) + 1.0) < 1e-15      # w = -1: (T, B, N) is left-handed, det -1
        back, _ = T.decode(frame, c)
        assert float((back - m).abs().max()) < 1e-15
    rgb = MG.quantise(0.5 * want.float().numpy() + 0.5)
    assert rgb[0] > 128 > rgb[1] and rgb[2] > 200


def test_w_from_the_definition_on_an_icosphere():
    """sign(cross(N, T) . (-dP/dv)) over the 960 corners: -1, the header's constant.  On the copy with its vertex normals negated the same
    expression is +1 on every corner: cross(N, T) is linear in N and T = normalise(s e1 - N (N . s e1)) does not change with N's sign, so
    the expression is odd in N and cannot be -1 for both.  The header says what the kernels do with such normals: w stays -1, and a reader
    that forms w cross(N, T) still decodes exactly what was encoded - held below."""
    v, f, _ = M.mesh_scene("sphere", 1)
    n = C.normals(v, f)
    fr = T.corner_frames(v, f, n)
    assert fr["ct"].shape == (960, 4) and bool(fr["keep"].all()) and not bool(fr["fallback"].any())
    w = T.derived_w(v, f, fr["cn"], fr["ct"])
    assert bool((w == -1).all()) and bool((fr["ct"][:, 3] == w).all())
    # tilted 0.3 rad off the face normals, both halves
    g = torch.Generator().manual_seed(0)
    axis = torch.nn.functional.normalize(torch.randn(n.shape[0], 3, generator=g, dtype=F64), dim=1)
    side = torch.nn.functional.normalize(torch.linalg.cross(n, axis), dim=1)
    tilted = math.cos(0.3) * n + math.sin(0.3) * side
    ft = T.corner_frames(v, f, tilted)
    assert bool((T.derived_w(v, f, ft["cn"], ft["ct"]) == -1).all())
    fneg = T.corner_frames(v, f, -n)
    assert torch.equal(fneg["ct"][:, :3], fr["ct"][:, :3]) and torch.equal(fneg["cn"], -fr["cn"]) and bool((fneg["ct"][:, 3] == -1).all())
    assert bool((T.derived_w(v, f, fneg["cn"], fneg["ct"]) == 1).all())
    m = torch.nn.functional.normalize(T.restated_object_map(64).double(), dim=1)
    enc = T.convert_map(f, v.shape[0], fneg["cn"], fneg["ct"], m, 64, True)
    dec = T.convert_map(f, v.shape[0], fneg["cn"], fneg["ct"], enc["map"], 64, False)
    assert float((dec["map"] - m)[enc["live"]].abs().max()) < 1e-12
    cnh, cth = MG.corner_frames_host(v, f, n)
    assert float(np.abs(cnh - fr["cn"].numpy()).max()) < 1e-7 and float(np.abs(cth - fr["ct"].numpy()).max()) < 1e-7
    assert float(np.abs(MG.vertex_normals_host(v, f) - n.numpy()).max()) < 1e-12


def test_invalid_faces_and_the_fallback_basis():
    v, f, n, _ = T.frame_case("degenerate")
    fr = T.corner_frames(v, f, n)
    assert fr["cn"][963:].tolist() == [[0, 0, 1]] * 3 and fr["ct"][963:].tolist() == [[1, 0, 0, -1]] * 3 and not bool(fr["valid"][963:].any())
    assert bool(fr["valid"][:963].all()) and bool(fr["keep"].all())
    v, f, n = T.fallback_face()
    fr, fr32 = T.corner_frames(v, f, n), T.corner_frames(v, f, n, F32)
    assert fr["fallback"].tolist() == fr32["fallback"].tolist() == [True, True, False]
    assert fr["cn"][:2].tolist() == [[0, 0, 1], [0, 0, -1]] and float((fr["cn"][2] - torch.tensor([0.6, 0.0, 0.8], dtype=F64)).abs().max()) < 1e-7
    assert fr["ct"][0].tolist() == [1, 0, 0, -1] and fr["ct"][1].tolist() == [1, 0, 0, -1]                # t1 of (0, 0, +-1)
    assert float((fr["ct"][2, :3] - torch.tensor([-0.8, 0.0, 0.6], dtype=F64)).abs().max()) < 1e-7        # (0, 0, .5) - N 0.4, normalised
    assert float(((fr["cn"] * fr["ct"][:, :3]).sum(1)).abs().max()) < 1e-15
    cnh, cth = MG.corner_frames_host(v, f, n)
    assert np.array_equal(cnh, fr["cn"].float().numpy()) and float(np.abs(cth - fr["ct"].numpy()).max()) < 1e-7


@pytest.mark.parametrize("tex", T.MAP_SIZES)
def test_round_trip_and_rigid_motion_of_the_restatement(tex):
    lv, lf, ln = T.low_mesh()
    m = torch.nn.functional.normalize(T.restated_object_map(tex).double(), dim=1)          # (the float32 map is of length 1 to 6e-8 only)
    fr = T.corner_frames(lv, lf, ln)
    enc = T.convert_map(lf, lv.shape[0], fr["cn"], fr["ct"], m, tex, True)
    live = enc["live"]
    assert torch.equal(enc["owner"], TX.texel_cells(320, tex)[0]) and bool((enc["map"][~live] == torch.tensor([0.0, 0.0, 1.0], dtype=F64)).all())
    assert float((enc["map"][live].norm(dim=1) - 1).abs().max()) < 1e-14
    dec = T.convert_map(lf, lv.shape[0], fr["cn"], fr["ct"], enc["map"], tex, False)
    trip = float((dec["map"] - m)[live].abs().max())
    print(f"R {tex}: round trip {trip:.3e}; |det| {float(enc['det'][live].abs().min()):.4f} .. {float(enc['det'][live].abs().max()):.4f}")
    assert trip < 1e-12
    # the mesh rotated (in fp64, not rounded): its frames decode the SAME tangent map to the rotated normals
    Q = T.rotation()
    assert float((Q @ Q.t() - torch.eye(3, dtype=F64)).abs().max()) < 1e-15 and float(Q.abs().min()) > 0.04 and float(Q.abs().max()) < 0.9          # about no axis of the frame
    fq = T.corner_frames(lv.double() @ Q.t(), lf, ln.double() @ Q.t())
    moved = T.convert_map(lf, lv.shape[0], fq["cn"], fq["ct"], enc["map"], tex, False)
    assert float((moved["map"] - m @ Q.t())[live].abs().max()) < 1e-12


# ---- the GLB ----------------------------------------------------------------------------------------------------------------------------------
def glb_inputs(R=32, seed=0):
    v, f = M.icosphere(0)
    g = torch.Generator().manual_seed(seed)
    tex, ao = torch.rand(R * R, 3, generator=g), torch.rand(R * R, generator=g) * 1.2 - 0.1
    tm = torch.nn.functional.normalize(torch.randn(R * R, 3, generator=g), dim=1)
    return v.numpy(), f.numpy(), tex.numpy(), tm.numpy(), ao.numpy(), R


@pytest.mark.parametrize("with_tm", (False, True))
@pytest.mark.parametrize("with_ao", (False, True))
def test_glb_against_the_specification(tmp_path, with_tm, with_ao):
    v, f, tex, tm, ao, R = glb_inputs()
    F = f.shape[0]
    path = str(tmp_path / "m.glb")
    size = MG.save_glb(path, v, f, tex, tangent_map=tm if with_tm else None, ao_map=ao if with_ao else None, tex_size=R)
    raw = open(path, "rb").read()
    assert size == len(raw)
    g = T.parse_glb(raw)                                     # magic, version, total length, chunk types, lengths and alignment
    assert set(g["json_pad"]) <= {0x20} and set(g["bin_pad"]) <= {0}
    js = g["json"]
    assert js["asset"]["version"] == "2.0" and js["scene"] == 0 and js["scenes"] == [{"nodes": [0]}] and len(js["nodes"]) == 1 and len(js["meshes"]) == 1
    node = js["nodes"][0]
    assert node["mesh"] == 0 and np.allclose(node["rotation"], [-math.sqrt(0.5), 0, 0, math.sqrt(0.5)], atol=1e-15)
    x, y, z, w = node["rotation"]                            # the quaternion as a matrix: (x, y, z) -> (x, z, -y)
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert np.allclose(Rm @ np.array([1.0, 2.0, 3.0]), [1.0, 3.0, -2.0], atol=1e-15)
    prims = js["meshes"][0]["primitives"]
    assert len(prims) == 1 and prims[0]["mode"] == 4 and "indices" not in prims[0] and prims[0]["material"] == 0
    att = prims[0]["attributes"]
    assert set(att) == {"POSITION", "NORMAL", "TANGENT", "TEXCOORD_0"}
    kinds = {"POSITION": "VEC3", "NORMAL": "VEC3", "TANGENT": "VEC4", "TEXCOORD_0": "VEC2"}
    for k, i in att.items():
        a = js["accessors"][i]
        assert a["count"] == 3 * F and a["type"] == kinds[k] and a["componentType"] == 5126
        assert js["bufferViews"][a["bufferView"]]["target"] == 34962
    for bv in js["bufferViews"]:
        assert bv["buffer"] == 0 and bv["byteOffset"] % 4 == 0 and bv["byteOffset"] + bv["byteLength"] <= js["buffers"][0]["byteLength"]
    pos, nrm, tan, uv = (T.glb_accessor(g, att[k]) for k in ("POSITION", "NORMAL", "TANGENT", "TEXCOORD_0"))
    assert np.array_equal(pos, v[f.reshape(-1)])
    pa = js["accessors"][att["POSITION"]]
    assert pa["min"] == pos.min(0).tolist() and pa["max"] == pos.max(0).tolist()
    assert float(np.abs(np.linalg.norm(nrm, axis=1) - 1).max()) < 1e-6 and float(np.abs(np.linalg.norm(tan[:, :3], axis=1) - 1).max()) < 1e-6
    assert set(tan[:, 3].tolist()) <= {-1.0, 1.0} and float(np.abs((nrm * tan[:, :3]).sum(1)).max()) < 1e-6
    vt = TX.face_uvs(F, R).reshape(-1, 2).numpy()
    assert np.array_equal(uv, ((vt + 0.5) / R).astype(np.float32))          # no flip: row y of the atlas is row y of the PNG from the top
    fr = T.corner_frames(torch.from_numpy(v), torch.from_numpy(f), C.normals(torch.from_numpy(v), torch.from_numpy(f)))
    assert float(np.abs(nrm - fr["cn"].numpy()).max()) < 1e-6 and float(np.abs(tan - fr["ct"].numpy()).max()) < 1e-6
    assert js["samplers"] == [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
    mat = js["materials"][0]
    assert mat["pbrMetallicRoughness"] == {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0} and mat["doubleSided"] is False
    assert ("normalTexture" in mat) == with_tm and ("occlusionTexture" in mat) == with_ao
    assert len(js["textures"]) == len(js["images"]) == 1 + with_tm + with_ao and all(t["sampler"] == 0 for t in js["textures"])
    q8 = lambda x: np.floor(np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)  # noqa: E731
    assert np.array_equal(T.glb_image(g, 0), q8(tex).reshape(R, R, 3))
    if with_tm:
        assert np.array_equal(T.glb_image(g, mat["normalTexture"]["index"]), q8(0.5 * tm + 0.5).reshape(R, R, 3))
    if with_ao:
        img = T.glb_image(g, mat["occlusionTexture"]["index"])
        assert img.shape == (R, R, 3) and np.array_equal(img, np.repeat(q8(ao).reshape(R, R, 1), 3, 2))
    # writer -> reader
    back = MG.read_glb(path)
    assert np.array_equal(back["verts"], pos) and np.array_equal(back["faces"], np.arange(3 * F).reshape(F, 3)) and np.array_equal(back["uv"], uv)
    assert np.array_equal(back["normals"], nrm) and np.array_equal(back["tangents"], tan) and back["tex_size"] == R
    assert float(np.abs(back["texture"] - np.clip(tex, 0, 1)).max()) <= 0.5 / 255 + 1e-6
    assert (back["tangent_map"] is None) == (not with_tm) and (back["ao_map"] is None) == (not with_ao)
    if with_tm:
        assert float(np.abs(back["tangent_map"] - tm).max()) <= 1.0 / 255 + 1e-6
    if with_ao:
        assert float(np.abs(back["ao_map"] - np.clip(ao, 0, 1)).max()) <= 0.5 / 255 + 1e-6


def test_glb_takes_given_frames_refuses_bad_maps_and_writes_an_empty_mesh(tmp_path):
    v, f, tex, tm, ao, R = glb_inputs()
    cn, ct = MG.corner_frames_host(v, f)
    ct2 = ct.copy()
    ct2[:, :3] = -ct2[:, :3]
    MG.save_glb(str(tmp_path / "a.glb"), v, f, tex, tex_size=R, corner_normals=cn, corner_tangents=ct2)
    assert np.array_equal(MG.read_glb(str(tmp_path / "a.glb"))["tangents"], ct2)
    MG.save_glb(str(tmp_path / "t.glb"), torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(tex))          # tensors, R from the texture
    assert MG.read_glb(str(tmp_path / "t.glb"))["tex_size"] == R
    for kw, what in ((dict(tangent_map=tm[:10]), "tangent map of 10"), (dict(ao_map=ao[:10]), "occlusion map of 10"), (dict(tex_size=31), "not 31 x 31"),
                     (dict(corner_normals=cn), "come together"), (dict(corner_normals=cn[:3], corner_tangents=ct[:3]), "3 corner normals")):
        with pytest.raises(ValueError, match=what):
            MG.save_glb(str(tmp_path / "bad.glb"), v, f, tex, **kw)
    with pytest.raises(ValueError, match="outside the vertex array"):
        MG.save_glb(str(tmp_path / "bad.glb"), v, np.array([[0, 1, 99]]), tex)
    with pytest.raises(ValueError, match="too small"):
        MG.save_glb(str(tmp_path / "bad.glb"), v, f, tex[:16 * 3].reshape(-1, 3)[:16], tex_size=4)
    for vv, ff in ((v, np.zeros((0, 3), np.int64)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))):
        MG.save_glb(str(tmp_path / "e.glb"), vv, ff, tex, tangent_map=tm, ao_map=ao)
        g = T.parse_glb(open(tmp_path / "e.glb", "rb").read())
        assert g["bin"] == b"" and "meshes" not in g["json"] and "mesh" not in g["json"]["nodes"][0]
        back = MG.read_glb(str(tmp_path / "e.glb"))
        assert back["verts"].shape == (0, 3) and back["faces"].shape == (0, 3) and back["texture"] is None
    with pytest.raises(ValueError, match="not a GLB"):
        open(tmp_path / "x.glb", "wb").write(b"not a glb file at all....")
        MG.read_glb(str(tmp_path / "x.glb"))


# ---- the script and the host API --------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_export_glb_options_parse():
    mod = _entry("export_glb")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh_50k_ao.obj", "-o", "out/gs/mesh_50k.glb"]))
    assert a == {"mesh": "out/gs/mesh_50k_ao.obj", "out": "out/gs/mesh_50k.glb", "high": None, "white_background": False, "texture_resolution": 1024,
                 "max_dist": None, "views": 8, "reso": 512, "radius": 2.0, "elevation": 0.0, "fov": 60.0, "render_orbit": 0, "json": None}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov"):
        assert a[k] == recon[k], k
    b = vars(ap.parse_args(["--mesh", "m.ply", "--high", "h.ply", "--render_orbit", "36", "--json", "s.json", "-w", "--texture_resolution", "2048"]))
    assert (b["high"], b["render_orbit"], b["json"], b["white_background"], b["texture_resolution"], b["out"]) == ("h.ply", 36, "s.json", True, 2048, None)
    with pytest.raises(SystemExit):
        ap.parse_args(["-o", "x.glb"])
    base = ["--mesh", "does/not/exist.obj"]
    for bad in (["--texture_resolution", "0"], ["--texture_resolution", "4097"], ["-o", "out.obj"], ["--render_orbit", "-1"], ["--reso", "0"], ["--views", "-1"],
                ["--max_dist", "-1"], ["--max_dist", "nan"], ["--json", "out.txt"], ["--high", "h.obj"]):
        with pytest.raises(SystemExit):                    # refused before anything is read
            mod.main(base + bad)
    with pytest.raises(SystemExit):
        mod.main(["--mesh", "does/not/exist.glb"])


def test_export_glb_finds_the_maps_of_its_input(tmp_path):
    from v3d_amd.recon import mesh_texture as MT
    mod = _entry("export_glb")
    v, f, tex, tm, ao, R = glb_inputs()
    vt = TX.face_uvs(f.shape[0], R).float()
    MT.save_textured_obj(str(tmp_path / "plain.obj"), v, f, vt, tex)
    MT.save_textured_obj(str(tmp_path / "two words.obj"), v, f, vt, tex, normal_map=tm, ao_map=ao)
    assert mod.map_of(str(tmp_path / "plain.obj"), "norm") is None and mod.map_of(str(tmp_path / "plain.obj"), "map_Ka") is None
    assert mod.map_of(str(tmp_path / "two words.obj"), "norm") == str(tmp_path / "two words_normal.png")
    assert mod.map_of(str(tmp_path / "two words.obj"), "map_Ka") == str(tmp_path / "two words_ao.png")
    n = mod.decode_normal_png(str(tmp_path / "two words_normal.png"), R)
    assert n.dtype == np.float32 and float(np.abs(np.linalg.norm(n, axis=1) - 1).max()) < 1e-6 and float(np.abs(n - tm).max()) < 2.0 / 255
    with pytest.raises(SystemExit, match="beside a texture"):
        mod.decode_normal_png(str(tmp_path / "two words_normal.png"), R + 1)
    # a map that the MTL names and that is not there: refused before anything is converted or written
    MT.save_textured_obj(str(tmp_path / "in.obj"), v, f, vt, tex, normal_map=tm, ao_map=ao)
    os.remove(tmp_path / "in_ao.png")
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit, match="in_ao.png"):
        mod.main(["--mesh", str(tmp_path / "in.obj"), "-o", str(tmp_path / "never.glb")])
    assert sorted(os.listdir(tmp_path)) == before


def test_host_api_refuses_bad_arguments_and_answers_the_empty_cases_without_a_launch():
    from v3d_amd.recon.cameras import orbit_cameras
    v, f = M.icosphere(0)
    none_f, none_v = torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3)
    up = torch.tensor([0.0, 0.0, 1.0])
    for vv, ff in ((v, none_f), (none_v, none_f)):
        cn, ct = MG.corner_frames(vv, ff, device="cpu")
        assert tuple(cn.shape) == (0, 3) and tuple(ct.shape) == (0, 4)
        for fn in (MG.to_tangent_space, MG.to_object_space):
            out = fn(vv, ff, torch.rand(64, 3), 8, device="cpu")
            assert tuple(out.shape) == (64, 3) and bool((out == up).all())
        cam = orbit_cameras(1, 2.0, 0.0, 60.0, 16)[0][0]
        lit = MG.prepare_lit_view(cam, vv, ff, 8, [0.1, 0.2, 0.3], device="cpu")
        img, nrm = MG.shade_lit(lit, torch.rand(64, 3))
        assert tuple(img.shape) == (3, 16, 16) and bool((img == torch.tensor([0.1, 0.2, 0.3]).view(3, 1, 1)).all()) and not nrm.any()
        with pytest.raises(ValueError, match="5 lights"):
            MG.shade_lit(lit, torch.rand(64, 3), lights=[((0, 0, 1), 1.0)] * 5)
        with pytest.raises(ValueError, match="no direction"):
            MG.shade_lit(lit, torch.rand(64, 3), lights=[((0, 0, 0), 1.0)])
        with pytest.raises(ValueError, match="albedo of 10"):
            MG.shade_lit(lit, torch.rand(10, 3))
    with pytest.raises(ValueError, match="tex_size 0"):
        MG.to_tangent_space(v, f, torch.rand(64, 3), 0, device="cpu")
    with pytest.raises(ValueError, match="map of 10 texels"):
        MG.to_tangent_space(v, f, torch.rand(10, 3), 8, device="cpu")
    with pytest.raises(ValueError, match="outside the vertex array"):
        MG.corner_frames(v, torch.tensor([[0, 1, 99]]), device="cpu")
    with pytest.raises(ValueError, match="12 vertices, 3 normals"):
        MG.corner_frames(v, f, normals=torch.zeros(3, 3), device="cpu")
    # the rig: unit directions that point from the surface towards the camera's side, in world space
    cam = orbit_cameras(4, 2.0, 15.0, 60.0, 16)[0][1]
    K, dirs, inten = MG._lights_arg(MG.camera_lights(cam), "t")
    assert K == 2 and float(np.abs(np.linalg.norm(dirs, axis=1) - 1).max()) < 1e-6 and inten.tolist() == [np.float32(0.85), np.float32(0.30)]
    forward = cam.world_view[:3, :3].double().numpy()[:, 2]                  # the camera's z axis in world space (view = world @ R)
    assert float(dirs[0] @ forward) < -0.5 and float(dirs[1] @ forward) < -0.3


# ---- the premises of the GPU cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.FRAME_CASES)
def test_premises_of_the_frame_cases(name):
    r64, r32 = T.frame_restatements(name)
    left_out = 1 - float(r64["keep"].float().mean())
    cn_err, ct_err = T.frame_errors(r32["cn"], r32["ct"], r64)
    print(f"{name}: {r64['cn'].shape[0]} corners, {100 * left_out:.3f} % left out, {int(r64['fallback'].sum())} on the fallback basis; float32 restatement "
          f"off by {cn_err:.3e} (normals), {ct_err:.3e} (tangents)")
    assert left_out <= T.EXCLUDE_MAX and left_out == 0
    assert torch.equal(r64["fallback"], r32["fallback"])
    if name == "first257":
        assert r64["cn"].shape[0] == 771
    if name in ("sphere", "degenerate"):
        assert cn_err > 0 and ct_err > 0          # the bar 4 x float32 means something


@pytest.mark.parametrize("source", ("baked", "constant"))
@pytest.mark.parametrize("tex", T.MAP_SIZES)
def test_premises_of_the_map_cases(tex, source):
    lv, lf, ln = T.low_mesh()
    m = T.restated_object_map(tex) if source == "baked" else T.constant_map(tex)
    fr = T.corner_frames(lv, lf, ln, F32)
    cn, ct = fr["cn"].float(), fr["ct"].float()
    enc = T.convert_map(lf, lv.shape[0], cn, ct, m, tex, True)
    dec = T.convert_map(lf, lv.shape[0], cn, ct, enc["map"].float(), tex, False)
    live = enc["live"]
    out_e, out_d = 1 - float(enc["keep"][live].float().mean()), 1 - float(dec["keep"][live].float().mean())
    det = enc["det"][live].abs()
    print(f"{source} R {tex}: {int(live.sum())} owned texels, {100 * out_e:.3f} % / {100 * out_d:.3f} % left out of encode / decode; |det| {float(det.min()):.4f} "
          f".. {float(det.max()):.4f}")
    assert out_e <= T.EXCLUDE_MAX and out_d <= T.EXCLUDE_MAX and out_e == out_d == 0
    assert float(det.min()) > 0.5                          # corner normals about 20 degrees apart: far from the 1e-12 rule
    # the rotated mesh
    fq = T.corner_frames(T.rotated(lv), lf, T.rotated(ln), F32)
    moved = T.convert_map(lf, lv.shape[0], fq["cn"].float(), fq["ct"].float(), enc["map"].float(), tex, False)
    assert 1 - float(moved["keep"][live].float().mean()) == 0


@pytest.mark.parametrize("view", T.LIT_VIEWS, ids=M.case_id)
def test_premises_of_the_lit_cases(view):
    vw = T.lit_view_restatement(view)
    albedo, tm, ao = T.random_maps(T.LIT_R)
    F = vw["faces"].shape[0]
    worst = 0.0
    for K in T.LIT_K:
        dirs, inten = T.light_arrays(K)
        for use_tm in (tm, None):
            r = T.shade_lit(vw["face_id"], vw["pix_w"], vw["pix_tex"], vw["pix_tw"], F, vw["cn"], vw["ct"], use_tm, albedo, ao, T.LIT_R, dirs, inten,
                            T.LIT_AMBIENT, T.LIT_BG)
            cov = r["covered"]
            worst = max(worst, 1 - float(r["keep"][cov].float().mean()))
            assert float((r["normals"].norm(dim=0)[cov] - 1).abs().max()) < 1e-12 and not r["normals"][:, ~cov].any()
            assert bool((r["image"][:, ~cov] == torch.tensor(T.LIT_BG, dtype=F64)[:, None]).all())
    cov = vw["face_id"] >= 0
    print(f"{M.case_id(view)}: {int(cov.sum())} of {cov.numel()} pixels covered, {100 * worst:.3f} % left out")
    assert 0.1 < float(cov.float().mean()) < 0.9 and worst == 0
    # without a map the normal is the interpolated vertex normal: within the faceting of the icosphere of the sphere's own normal
    r = T.shade_lit(vw["face_id"], vw["pix_w"], vw["pix_tex"], vw["pix_tw"], F, vw["cn"], vw["ct"], None, albedo, None, T.LIT_R, [], [], 1.0, T.LIT_BG)
    img = TX.shade(vw["pix_tex"], vw["pix_tw"], albedo, T.LIT_BG)
    assert float((r["image"] - img).abs().max()) < 1e-12          # K = 0, ambient 1, no occlusion: the albedo alone, as v3d_recon_tex_shade


def test_premises_of_the_end_to_end_scene():
    """The figures tests/test_mesh_tangent_gpu.py quotes: (a) vertex normals, (b) object-space map, (c) tangent-space map, in degrees, on the
    restatements alone.  The tangent path keeps the bake's value."""
    e = T.e2e_restatement()
    print(f"end to end on the restatement: vertex normals {e['before']:.4f}, object-space map {e['object']:.4f}, tangent-space map {e['tangent']:.4f} "
          f"(float32 {e['tangent32']:.4f}) degrees")
    assert e["before"] - e["object"] > 4.0
    assert abs(e["before"] - E2E_RESTATEMENT["before"]) < 0.02 and abs(e["object"] - E2E_RESTATEMENT["object"]) < 0.02
    assert abs(e["tangent"] - E2E_RESTATEMENT["tangent"]) < 0.002 and abs(e["tangent32"] - e["tangent"]) <= E2E_RESTATEMENT["float32"]
    assert e["before"] - e["tangent"] >= 0.9 * (e["before"] - e["object"])


# measured by test_premises_of_the_end_to_end_scene (degrees); "float32": a cap on |tangent32 - tangent|
E2E_RESTATEMENT = {"before": 5.9633, "object": 1.1634, "tangent": 1.1606, "float32": 1e-3}
