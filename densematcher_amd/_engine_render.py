"""
MatchEngine, textured-mesh rendering: the hard-Phong views of a ragged batch of raw meshes in ONE device call (dm_render_phong).
"""
import types

import numpy as np
import torch

from . import _lib
from ._operands import (host_ptr, image_frame, pad_stack, ptr as _ptr, render_colour, render_corners, render_normals, render_points, render_texture)

AMBIENT, DIFFUSE, SPECULAR, BACKGROUND, SHININESS = (0.6, 0.6, 0.6), (0.4, 0.4, 0.5), (0.01, 0.01, 0.01), (1.0, 1.0, 1.0), 64.0


def shade_params(ambient_color, diffuse_color, specular_color, background_color, shininess, who):
    """the 13 floats of a call: ambient, diffuse, specular, background, shininess"""
    s = float(shininess)
    if not (np.isfinite(s) and s >= 0.0):
        raise ValueError(f"{who}: shininess must be a finite number >= 0")
    return np.concatenate([render_colour(ambient_color, who, "ambient_color"), render_colour(diffuse_color, who, "diffuse_color"),
                           render_colour(specular_color, who, "specular_color"), render_colour(background_color, who, "background_color"),
                           np.asarray([s], np.float32)]).astype(np.float32)


class _RenderOps:
    def render_phong(self, verts_list, faces_list, cameras_list, H, W, textures_list=None, normals_list=None, light_list=None,
                     ambient_color=AMBIENT, diffuse_color=DIFFUSE, specular_color=SPECULAR, shininess=SHININESS, background_color=BACKGROUND,
                     focal_length=1.0, planes=None):
        """run_rendering of the reference (render.py:13-54) for a ragged batch of meshes in ONE device call: verts_list[b] (n_b, 3),
        faces_list[b] (m_b, 3), cameras_list[b] = (R (views_b, 3, 3), T (views_b, 3)); textures_list[b]: None (white), ("vertex",
        colours (n_b, 3)) or ("uv", map (Ht, Wt, 3), verts_uvs (n_uv, 2), faces_uvs (m_b, 3)), maps of any sizes; normals_list[b]:
        optional vertex normals (n_b, 3) in place of the area-weighted ones; light_list[b]: optional light locations (views_b, 3), the
        camera centres by default.  planes: None, torch.float32 or torch.float16 -- also return the RGB planes (views_b, 3, H, W).
        Returns a namespace of per-mesh lists: images (views_b, H, W, 4) fp32, zbuf (views_b, H, W) fp32 (-1: background), pix2face
        (views_b, H, W) int32 (-1: background), normals (n_b, 3) fp64, planes (or None); and padded = (rgba, zbuf, pix2face) of the
        whole call, (B, views, H, W, ...)."""
        who = "render_phong"
        m = self._lift_meshes(verts_list, faces_list, cameras_list, who)
        Bn, N, nt, Vw = m["B"], m["N"], m["nt"], m["Vw"]
        H, W = image_frame(H, W, focal_length, who)
        if planes not in (None, torch.float32, torch.float16):
            raise ValueError(f"{who}: planes must be None, torch.float32 or torch.float16")
        for name, lst in (("textures_list", textures_list), ("normals_list", normals_list), ("light_list", light_list)):
            if lst is not None and len(lst) != Bn:
                raise ValueError(f"{who}: {name}: one entry (or None) per mesh")
        shade = shade_params(ambient_color, diffuse_color, specular_color, background_color, shininess, who)
        _, faces, Rh, Th = m["host"]
        # ---- corners, normals, lights, textures: checked on the host, then one upload each
        ptrs, incs, keep = [], [], []
        table = np.zeros((Bn, 8), np.int64)
        n_inc = 3 * nt
        given = np.zeros(Bn, np.int32)
        normals = torch.zeros((Bn, N, 3), dtype=torch.float64, device=self.device)
        lights = None if light_list is None or all(x is None for x in light_list) else np.zeros((Bn, Vw, 3))
        for b in range(Bn):
            tag = f"{who}: mesh {b}"
            n, nf, nw = m["n_verts"][b], m["n_faces"][b], m["n_views"][b]
            p, f = render_corners(faces[b], n)
            ptrs.append(np.concatenate((p, np.full(N - n, p[-1], np.int32)))), incs.append(f)
            nrm = render_normals(None if normals_list is None else normals_list[b], n, tag)
            if nrm is not None:
                normals[b, :n] = torch.from_numpy(nrm).to(self.device)
                given[b] = 1
            if lights is not None:
                pts = render_points(light_list[b], nw, tag, "light_location")
                if pts is None:                                  # the camera centre C = -T R^T
                    pts = -np.einsum("vk,vjk->vj", Th[b], Rh[b])
                lights[b, :nw] = pts
            t = render_texture(None if textures_list is None else textures_list[b], n, nf, tag)
            if t[0] == 1:
                col = self._dev(t[1], torch.float32, "colours")
                keep.append(col)
                table[b] = (1, col.data_ptr(), n, 3, 0, 0, 0, 0)
            elif t[0] == 2:
                tmap, uvs, fuv = self._dev(t[1], torch.float32, "map"), self._dev(t[2], torch.float32, "verts_uvs"), self._dev(t[3], torch.int32, "faces_uvs")
                keep += [tmap, uvs, fuv]
                table[b] = (2, tmap.data_ptr(), tmap.shape[0], tmap.shape[1], uvs.data_ptr(), fuv.data_ptr(), uvs.shape[0], fuv.shape[0])
        self._check_stream()
        inc_ptr = self._dev(np.stack(ptrs), torch.int32, "inc_ptr")
        inc_face = self._dev(pad_stack(incs, (n_inc,), -1, np.int32), torch.int32, "inc_face")
        given_d = self._dev(given, torch.int32, "normals_given") if given.any() else None
        lights_d = None if lights is None else self._dev(lights, torch.float64, "light")
        table_d = self._dev(table, torch.int64, "tex")
        rgba = torch.empty((Bn, Vw, H, W, 4), dtype=torch.float32, device=self.device)
        zbuf = torch.empty((Bn, Vw, H, W), dtype=torch.float32, device=self.device)
        p2f = torch.empty((Bn, Vw, H, W), dtype=torch.int32, device=self.device)
        pl = None if planes is None else torch.empty((Bn, Vw, 3, H, W), dtype=planes, device=self.device)
        self._chk(self.lib.dm_render_phong(self.ctx, Bn, N, nt, Vw, H, W, _ptr(m["verts"]), _ptr(m["tri"]), _ptr(m["nv"]), _ptr(m["R"]), _ptr(m["T"]),
                                           _ptr(m["nw"]), float(focal_length), _ptr(inc_ptr), _ptr(inc_face), n_inc, _ptr(given_d), _ptr(normals),
                                           _ptr(table_d), _ptr(lights_d), host_ptr(shade), _ptr(rgba), _ptr(zbuf), _ptr(p2f), _ptr(pl),
                                           _lib.DM_F16 if planes == torch.float16 else _lib.DM_F32))
        per = lambda t: [t[b, :w] for b, w in enumerate(m["n_views"])]
        return types.SimpleNamespace(images=per(rgba), zbuf=per(zbuf), pix2face=per(p2f), planes=None if pl is None else per(pl),
                                     normals=[normals[b, :n] for b, n in enumerate(m["n_verts"])], padded=(rgba, zbuf, p2f))
