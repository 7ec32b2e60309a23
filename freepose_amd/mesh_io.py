"""Triangle-mesh container + Wavefront OBJ/MTL reader (the reference uses trimesh.load(path, force='mesh'),
scripts/dino_inference_video.py:93-101, scripts/render_templates.py:58-66; trimesh is not a dependency here) + PLY reader for the BOP
ground-truth models (bop_toolkit_lib/inout.py:504-537 load_mesh).

Appearance, in the order the rasteriser uses it:
  * per-corner texture coordinates `uv` [F,3,2] + diffuse `texture` [h,w,3] (+ material factor `kd`) -> per-fragment texture
    sampling (what pyrender.Mesh.from_trimesh renders for a TextureVisuals mesh, renderer.py:43-45);
  * per-vertex colours (`v x y z r g b` records, trimesh ColorVisuals);
  * white.
Several materials (`usemtl` groups) are packed into one atlas, like trimesh's concatenation under force='mesh': textures are
stacked vertically (each scaled to the widest one with nearest sampling), untextured materials become solid Kd patches, and a
face's coordinates are moved into its material's band (REPEAT addressing inside a band is lost for faces that span more than
one texture period — the same restriction as trimesh's packer).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np


@dataclass
class TriMesh:
    vertices: np.ndarray                          # [V,3] float
    faces: np.ndarray                             # [F,3] int
    vertex_colors: Optional[np.ndarray] = None    # [V,3] uint8
    uv: Optional[np.ndarray] = None               # [F,3,2] float32, OBJ convention (v up)
    texture: Optional[np.ndarray] = None          # [h,w,3] uint8, rows top to bottom
    kd: Optional[np.ndarray] = None               # [3] float32 diffuse factor applied to the texel
    vertices_f64: Optional[np.ndarray] = None     # [V,3] the vertices as parsed, before the rounding to float32 (load_obj; chamfer clouds)

    @property
    def pts(self):                       # the key the BOP toolkit's model dictionaries use (inout.load_mesh: model['pts'])
        return self.vertices

    def apply_scale(self, s: float):     # trimesh-compatible (reference mutates the mesh, online_pose_estimator.py:60,64)
        self.vertices = self.vertices * s
        if self.vertices_f64 is not None:
            self.vertices_f64 = self.vertices_f64 * s
        return self

    def sample(self, n: int, seed=None) -> np.ndarray:
        """n points [n,3] float64 on the surface: triangles drawn with probability proportional to their area, then uniform
        barycentric coordinates (the square-root-free fold of the unit square), all from numpy.random.default_rng(seed) (or a
        Generator passed as `seed`).  trimesh-compatible call (`mesh.sample(10000)`, tracking_refiner.py:103), but trimesh's own
        random stream is NOT reproduced: the same surface distribution, other points."""
        rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
        V = np.asarray(self.vertices_f64 if self.vertices_f64 is not None else self.vertices, dtype=np.float64)
        F = np.asarray(self.faces, dtype=np.int64)
        a, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
        area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
        if not len(F) or not area.sum() > 0:
            raise ValueError("TriMesh.sample: the mesh has no surface (no faces, or all of zero area)")
        tri = rng.choice(len(F), size=int(n), p=area / area.sum())
        uv = rng.random((int(n), 2))
        fold = uv.sum(1) > 1.0
        uv[fold] = 1.0 - uv[fold]
        return a[tri] + uv[:, :1] * e1[tri] + uv[:, 1:] * e2[tri]

    def copy(self):
        c = lambda a: None if a is None else np.array(a, copy=True)   # noqa: E731
        return TriMesh(c(self.vertices), c(self.faces), c(self.vertex_colors), c(self.uv), c(self.texture), c(self.kd), c(self.vertices_f64))


def mesh_appearance(mesh) -> dict:
    """keyword arguments for ops.Mesh from a TriMesh or a trimesh-like object: {'colors'} | {'uv','texture','kd'} | {}"""
    faces = np.asarray(mesh.faces)
    n_v = len(np.asarray(mesh.vertices))
    uv, tex, kd = getattr(mesh, "uv", None), getattr(mesh, "texture", None), getattr(mesh, "kd", None)
    if uv is not None and tex is not None:
        return {"uv": np.asarray(uv, np.float32).reshape(-1, 3, 2), "texture": np.asarray(tex)[:, :, :3].astype(np.uint8), "kd": kd}
    vis = getattr(mesh, "visual", None)
    if vis is not None and getattr(vis, "uv", None) is not None:       # trimesh TextureVisuals: per-vertex uv + material image
        mat = getattr(vis, "material", None)
        img = getattr(mat, "image", None)
        if img is None:
            img = getattr(mat, "baseColorTexture", None)
        if img is not None:
            tex = np.asarray(img.convert("RGB") if hasattr(img, "convert") else img)[:, :, :3].astype(np.uint8)
            vuv = np.asarray(vis.uv, np.float32)
            if len(vuv) == n_v:
                fac = getattr(mat, "diffuse", None)
                if fac is None:
                    fac = getattr(mat, "baseColorFactor", None)
                kd = None
                if fac is not None:
                    fac = np.asarray(fac, np.float32).reshape(-1)[:3]
                    kd = fac / 255.0 if fac.max() > 1.0 else fac
                return {"uv": vuv[faces.reshape(-1)].reshape(-1, 3, 2), "texture": tex, "kd": kd}
        if hasattr(vis, "to_color"):                                    # textured visual without a usable image
            vis = vis.to_color()
    c = getattr(mesh, "vertex_colors", None)
    if c is None and vis is not None:
        c = getattr(vis, "vertex_colors", None)
    if c is not None:
        c = np.asarray(c)
        if c.ndim == 2 and len(c) == n_v:
            return {"colors": c[:, :3].astype(np.uint8)}
    return {}


def mesh_arrays(mesh):
    """(vertices f32 [V,3], faces i32 [F,3], appearance dict) from a TriMesh or any trimesh-like object."""
    v = np.asarray(mesh.vertices, dtype=np.float32)
    f = np.asarray(mesh.faces, dtype=np.int32)
    return v, f, mesh_appearance(mesh)


def device_mesh(mesh):
    """upload a TriMesh / trimesh-like object: ops.Mesh with its textured, vertex-coloured or plain appearance"""
    from freepose_amd import ops
    v, f, app = mesh_arrays(mesh)
    return ops.Mesh(v, f, **app)


def mesh_cloud_f64(mesh) -> np.ndarray:
    """[V,3] float64 vertex cloud for the chamfer errors: the unrounded vertices where the reader kept them (TriMesh.vertices_f64)"""
    v = mesh.vertices_f64 if isinstance(mesh, TriMesh) and mesh.vertices_f64 is not None else mesh.vertices
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).reshape(-1, 3)


def mesh_signature(mesh):
    """cheap content check for device-mesh caches: meshes are mutated in place by the pipeline (apply_scale,
    online_pose_estimator.py:60,64) and ids are recycled, so identity alone is not a key"""
    v = np.asarray(mesh.vertices)
    f = np.asarray(mesh.faces)
    return (v.shape, f.shape, float(np.abs(v).sum()), float(v[0].sum()) if len(v) else 0.0, int(f[-1].sum()) if len(f) else 0)


# ---- OBJ / MTL -------------------------------------------------------------------------------------------------------
def _read_mtl(mtl_path: Path) -> dict:
    """material name -> {'kd': [3] float, 'map': Path | None}"""
    mats, cur = {}, None
    if not mtl_path.is_file():
        return mats
    for line in mtl_path.read_text(errors="ignore").splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "newmtl":
            cur = " ".join(t[1:])
            mats[cur] = {"kd": None, "map": None}
        elif cur is not None and t[0] == "Kd" and len(t) >= 4:
            mats[cur]["kd"] = np.array([float(x) for x in t[1:4]], np.float32)
        elif cur is not None and t[0] == "map_Kd":
            p = mtl_path.parent / t[-1]
            mats[cur]["map"] = p if p.is_file() else None
    return mats


def _load_image(p: Path):
    try:
        from PIL import Image
        im = Image.open(p)
        if im.mode in ("LA", "1", "P", "L", "RGBA", "I;16"):   # fix_mesh_texture's conversions (render_templates.py:13-25) and more
            im = im.convert("RGB")
        return np.asarray(im.convert("RGB"))
    except Exception:
        return None


def load_obj(path) -> TriMesh:
    mesh, v64 = _load_obj(Path(path))
    if len(v64) == len(mesh.vertices):
        mesh.vertices_f64 = v64
    return mesh


def _load_obj(path: Path):
    vs, vcol, vts, faces, face_vt, face_mat = [], [], [], [], [], []
    mtllib, cur_mat = None, None
    for line in path.read_text(errors="ignore").splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            vs.append([float(x) for x in t[1:4]])
            if len(t) >= 7:
                vcol.append([float(x) for x in t[4:7]])
        elif t[0] == "vt":
            vts.append([float(t[1]), float(t[2]) if len(t) > 2 else 0.0])
        elif t[0] == "f":
            idx = [p.split("/") for p in t[1:]]
            vi = [int(p[0]) for p in idx]
            ti = [int(p[1]) if len(p) > 1 and p[1] else 0 for p in idx]
            vi = [i - 1 if i > 0 else len(vs) + i for i in vi]
            ti = [i - 1 if i > 0 else (len(vts) + i if i < 0 else -1) for i in ti]
            for k in range(1, len(vi) - 1):     # fan triangulation
                faces.append([vi[0], vi[k], vi[k + 1]])
                face_vt.append([ti[0], ti[k], ti[k + 1]])
                face_mat.append(cur_mat)
        elif t[0] == "mtllib":
            mtllib = " ".join(t[1:])
        elif t[0] == "usemtl":
            cur_mat = " ".join(t[1:])
    V = np.asarray(vs, dtype=np.float32).reshape(-1, 3)
    V64 = np.asarray(vs, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    if len(vcol) == len(vs) and vs:
        c = np.asarray(vcol, dtype=np.float32)
        colors = np.clip(c * (255.0 if c.max() <= 1.0 else 1.0) + 0.5, 0, 255).astype(np.uint8)
        return TriMesh(V, F, colors), V64
    mats = _read_mtl(path.parent / mtllib) if mtllib else {}
    if not mats or not len(F):
        return TriMesh(V, F, None), V64
    return _with_materials(V, F, np.asarray(vts, np.float32).reshape(-1, 2), np.asarray(face_vt, np.int64).reshape(-1, 3),
                           face_mat, mats), V64


def _with_materials(V, F, vts, face_vt, face_mat, mats) -> TriMesh:
    used = []
    for m in face_mat:
        if m not in used:
            used.append(m)
    if None in used and len(mats) == 1:         # faces before any usemtl take the only material
        only = next(iter(mats))
        face_mat = [only if m is None else m for m in face_mat]
        used = [only if m is None else m for m in used]
        used = list(dict.fromkeys(used))
    images = {}
    for m in used:
        info = mats.get(m)
        img = _load_image(info["map"]) if info and info["map"] is not None else None
        images[m] = img
    has_uv = len(vts) > 0
    if len(used) == 1 and images[used[0]] is not None and has_uv:
        m = used[0]
        ok = (face_vt >= 0).all(axis=1)
        uv = np.zeros((len(F), 3, 2), np.float32)
        uv[ok] = vts[face_vt[ok]]
        kd = mats[m]["kd"] if m in mats else None
        # a textured material's Kd multiplies the texel (baseColorFactor); exporters write 0 0 0 next to map_Kd when they mean "texture only"
        if kd is not None and float(kd.max()) <= 0.0:
            kd = None
        return TriMesh(V, F, None, uv, images[m], kd)
    if all(images[m] is None for m in used):
        kds = [mats[m]["kd"] if (m in mats and mats[m]["kd"] is not None) else np.ones(3, np.float32) for m in used]
        if len(used) == 1:                       # one untextured material: a uniform colour
            col = np.clip(kds[0] * 255.0 + 0.5, 0, 255).astype(np.uint8)
            return TriMesh(V, F, np.tile(col, (len(V), 1)))
    # ---- atlas: one band per material, stacked vertically ---------------------------------------------------------
    width = max([images[m].shape[1] for m in used if images[m] is not None] + [4])
    bands, tops = [], {}
    y = 0
    for m in used:
        img = images[m]
        if img is None:
            kd = mats[m]["kd"] if (m in mats and mats[m]["kd"] is not None) else np.ones(3, np.float32)
            band = np.tile(np.clip(kd * 255.0 + 0.5, 0, 255).astype(np.uint8), (4, width, 1))
        else:
            h0, w0 = img.shape[:2]
            if w0 != width:                      # nearest resample to the common width (keeps the aspect ratio)
                h1 = max(1, int(round(h0 * width / w0)))
                yy = np.minimum((np.arange(h1) * h0 / h1).astype(int), h0 - 1)
                xx = np.minimum((np.arange(width) * w0 / width).astype(int), w0 - 1)
                img = img[yy][:, xx]
            band = img[:, :, :3]
            kd = mats[m]["kd"] if m in mats else None
            if kd is not None and float(kd.max()) > 0.0 and not np.allclose(kd, 1.0):
                band = np.clip(band.astype(np.float32) * kd + 0.5, 0, 255).astype(np.uint8)
        tops[m] = (y, band.shape[0])
        bands.append(band)
        y += band.shape[0]
    atlas = np.concatenate(bands, axis=0)
    H = atlas.shape[0]
    uv = np.zeros((len(F), 3, 2), np.float32)
    for i in range(len(F)):
        top, hb = tops[face_mat[i]]
        if images[face_mat[i]] is None or not has_uv or (face_vt[i] < 0).any():
            u, v = np.full(3, 0.5, np.float32), np.full(3, 0.5, np.float32)
        else:
            t = vts[face_vt[i]]
            u = t[:, 0] - np.floor(t[:, 0].min())
            v = t[:, 1] - np.floor(t[:, 1].min())
            u, v = np.clip(u, 0.0, 1.0), np.clip(v, 0.0, 1.0)
        # rows of the band, half a texel inside so that bilinear taps stay in the band
        vy = top + 0.5 + (1.0 - v) * (hb - 1.0)
        uv[i, :, 0] = u
        uv[i, :, 1] = 1.0 - vy / H
    return TriMesh(V, F, None, uv, atlas, None)


# ---- PLY ---------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def load_ply(path) -> TriMesh:
    """PLY as the BOP datasets ship their models: `ascii` or `binary_little_endian`, a vertex element (x y z, optionally red green
    blue, anything else is skipped) and a face element of triangles.  Vertices stay float64 (`.pts`, like inout.load_mesh)."""
    data = Path(path).read_bytes()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data[data.index(b"\n", end) + 1:]
    fmt, elements = None, []                     # elements: [name, count, [(property name, dtype) | (name, count dtype, item dtype)]]
    for line in data[:end].decode("ascii", errors="ignore").splitlines()[1:]:
        t = line.split()
        if not t or t[0] == "comment":
            continue
        if t[0] == "format":
            fmt = t[1]
        elif t[0] == "element":
            elements.append([t[1], int(t[2]), []])
        elif t[0] == "property" and elements:
            if t[1] == "list":
                elements[-1][2].append((t[4], _PLY_TYPES[t[2]], _PLY_TYPES[t[3]]))
            else:
                elements[-1][2].append((t[2], _PLY_TYPES[t[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format '{fmt}' (ascii and binary_little_endian are read)")
    tokens = body.split() if fmt == "ascii" else None
    pos = 0
    verts, colors, faces = None, None, np.zeros((0, 3), np.int32)
    for name, count, props in elements:
        has_list = any(len(p) == 3 for p in props)
        if name == "face":
            if len(props) < 1 or len(props[0]) != 3:
                raise ValueError(f"{path}: face element without a leading vertex-index list")
            if fmt == "ascii":
                rows = []
                for _ in range(count):
                    k = int(tokens[pos])
                    if k != 3:
                        raise ValueError(f"{path}: only triangular faces are read (found a face with {k} corners)")
                    rows.append([int(x) for x in tokens[pos + 1:pos + 4]])
                    pos += 4
                    for extra in props[1:]:              # e.g. a texcoord list after the indices
                        pos += (int(tokens[pos]) + 1) if len(extra) == 3 else 1
                faces = np.asarray(rows, np.int32).reshape(-1, 3)
            else:
                if len(props) == 1:                      # the common case in one step
                    rec = np.dtype([("k", "<" + props[0][1]), ("v", "<" + props[0][2], (3,))])
                    a = np.frombuffer(body, dtype=rec, count=count, offset=pos)
                    if count and (a["k"] != 3).any():
                        raise ValueError(f"{path}: only triangular faces are read")
                    faces = a["v"].astype(np.int32)
                    pos += rec.itemsize * count
                else:
                    rows = []
                    for _ in range(count):
                        for j, pr in enumerate(props):
                            if len(pr) == 3:
                                k = int(np.frombuffer(body, "<" + pr[1], 1, pos)[0])
                                pos += np.dtype(pr[1]).itemsize
                                v = np.frombuffer(body, "<" + pr[2], k, pos)
                                pos += np.dtype(pr[2]).itemsize * k
                                if j == 0:
                                    if k != 3:
                                        raise ValueError(f"{path}: only triangular faces are read")
                                    rows.append(v.astype(np.int32))
                            else:
                                pos += np.dtype(pr[1]).itemsize
                    faces = np.asarray(rows, np.int32).reshape(-1, 3)
        elif has_list:
            raise ValueError(f"{path}: list property in element '{name}'")
        else:
            names = [p[0] for p in props]
            if fmt == "ascii":
                a = np.asarray(tokens[pos:pos + count * len(props)], dtype=np.float64).reshape(count, len(props))
                pos += count * len(props)
                col = {n: a[:, i] for i, n in enumerate(names)}
            else:
                rec = np.dtype([(n, "<" + d) for n, d in props])
                a = np.frombuffer(body, dtype=rec, count=count, offset=pos)
                pos += rec.itemsize * count
                col = {n: a[n] for n in names}
            if name == "vertex":
                verts = np.stack([np.asarray(col[k], np.float64) for k in ("x", "y", "z")], axis=1)
                if all(k in col for k in ("red", "green", "blue")):
                    colors = np.stack([np.asarray(col[k]) for k in ("red", "green", "blue")], axis=1).astype(np.uint8)
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    return TriMesh(verts, faces, colors)


def load_mesh(path) -> TriMesh:
    """by extension: .ply (BOP models) or .obj (retrieved meshes)"""
    return load_ply(path) if str(path).lower().endswith(".ply") else load_obj(path)
