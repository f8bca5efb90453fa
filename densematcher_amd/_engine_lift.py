"""
MatchEngine, multi-view feature lifting: the visibility of a batch of simplified meshes in their views (dm_raster_pix2face) and the
per-vertex mean of the per-view feature maps (dm_lift_features).
"""
import numpy as np
import torch

from . import _lib
from ._operands import image_frame, lift_cameras, lift_mesh, lift_pix2face, pad_stack, ptr as _ptr

MAX_VIEWS = 64


class _LiftOps:
    # ------------------------------------------------------------- operands
    def _lift_meshes(self, verts_list, faces_list, cameras_list, who):
        """the meshes and cameras of a call, checked on the host and padded on the device"""
        Bn = len(verts_list)
        if Bn == 0 or len(faces_list) != Bn or len(cameras_list) != Bn:
            raise ValueError(f"{who}: one vertex array, one face array and one (R, T) pair per mesh")
        V, F, R, T = [], [], [], []
        for b in range(Bn):
            v, f = lift_mesh(verts_list[b], faces_list[b], f"{who}: mesh {b}")
            r, t = lift_cameras(cameras_list[b], f"{who}: mesh {b}", MAX_VIEWS)
            V.append(v), F.append(f.astype(np.int32)), R.append(r), T.append(t)
        n_verts, n_views = [v.shape[0] for v in V], [r.shape[0] for r in R]
        N, nt, Vw = max(n_verts), max(f.shape[0] for f in F), max(n_views)
        m = {"B": Bn, "N": N, "nt": nt, "Vw": Vw, "n_verts": n_verts, "n_views": n_views, "n_faces": [f.shape[0] for f in F], "host": (V, F, R, T),
             "verts": self._dev(pad_stack(V, (N, 3), 0.0, np.float64), torch.float64, "verts"),
             "tri": self._dev(pad_stack(F, (nt, 3), -1, np.int32), torch.int32, "tri"),
             "R": self._dev(pad_stack(R, (Vw, 3, 3), 0.0, np.float64), torch.float64, "R"),
             "T": self._dev(pad_stack(T, (Vw, 3), 0.0, np.float64), torch.float64, "T"),
             "nv": self._dev(np.asarray(n_verts, np.int32), torch.int32, "n_verts") if min(n_verts) < N else None,
             "nw": self._dev(np.asarray(n_views, np.int32), torch.int32, "n_views") if min(n_views) < Vw else None}
        return m

    def _lift_raster(self, m, H, W, focal_length, pix2face_list, who):
        """dm_raster_pix2face on the meshes m: (proj (B,Vw,N,4), pix2face (B,Vw,H,W), vis (B,Vw,N) uint8)"""
        H, W = image_frame(H, W, focal_length, who)
        Bn, N, Vw = m["B"], m["N"], m["Vw"]
        p2f = torch.full((Bn, Vw, H, W), -1, dtype=torch.int32, device=self.device)
        given = None
        if pix2face_list is not None:
            if len(pix2face_list) != Bn:
                raise ValueError(f"{who}: pix2face: one entry (or None) per mesh")
            flags = np.zeros(Bn, np.int32)
            for b, g in enumerate(pix2face_list):
                if g is None:
                    continue
                g = lift_pix2face(g, m["n_views"][b], m["n_faces"][b], f"{who}: mesh {b}")
                if tuple(g.shape[1:]) != (H, W):
                    raise ValueError(f"{who}: mesh {b}: pix2face must be ({m['n_views'][b]}, {H}, {W}) integers")
                p2f[b, :g.shape[0]] = g.to(device=self.device, dtype=torch.int32)
                flags[b] = 1
            given = self._dev(flags, torch.int32, "given") if flags.any() else None
        proj = torch.empty((Bn, Vw, N, 4), dtype=torch.float64, device=self.device)
        vis = torch.empty((Bn, Vw, N), dtype=torch.uint8, device=self.device)
        self._chk(self.lib.dm_raster_pix2face(self.ctx, Bn, N, m["nt"], Vw, H, W, _ptr(m["verts"]), _ptr(m["tri"]), _ptr(m["nv"]), _ptr(m["R"]),
                                              _ptr(m["T"]), _ptr(m["nw"]), float(focal_length), _ptr(given), _ptr(proj), _ptr(p2f), _ptr(vis)))
        return proj, p2f, vis

    # ------------------------------------------------------------- public
    def raster_visibility(self, verts_list, faces_list, cameras_list, H, W, focal_length=1.0):
        """The visibility of get_features_per_vertex (reference projection.py:60-62,94-101) for a ragged batch of meshes in ONE device
        call.  verts_list[b] (n_b, 3), faces_list[b] (m_b, 3), cameras_list[b] = (R (views_b, 3, 3), T (views_b, 3)) in pytorch3d's
        row-vector convention.  Returns (pix2face, visible): per mesh an int32 (views_b, H, W) tensor (-1: background) and a bool
        (views_b, n_b) mask of the vertices that belong to a face owning a pixel AND project strictly inside the frame."""
        m = self._lift_meshes(verts_list, faces_list, cameras_list, "raster_visibility")
        proj, p2f, vis = self._lift_raster(m, H, W, focal_length, None, "raster_visibility")
        seen = vis.bool() & (proj[..., 3] != 0)
        return ([p2f[b, :w] for b, w in enumerate(m["n_views"])],
                [seen[b, :w, :n] for b, (w, n) in enumerate(zip(m["n_views"], m["n_verts"]))])

    def lift_features(self, fts_list, verts_list, faces_list, cameras_list, pix2face_list=None, return_counts=False, focal_length=1.0):
        """get_features_per_vertex with fts given (reference projection.py:27-130) for a ragged batch of meshes: two device calls.
        fts_list[b]: (views_b, C, H, W) fp16 or fp32 feature maps, any strides (NCHW, channels-last, a view of a larger buffer): they
        are read where they lie.  pix2face_list[b] (optional, None per mesh to rasterise here): an integer (views_b, H, W) pix2face of
        the simplified mesh from any rasteriser; it replaces the raster pass for that mesh.
        Returns a list of (n_b, C) fp32 device tensors (with return_counts: also the list of (n_b,) int32 numbers of views per vertex)."""
        m = self._lift_meshes(verts_list, faces_list, cameras_list, "lift_features")
        Bn = m["B"]
        if len(fts_list) != Bn:
            raise ValueError("lift_features: one stack of feature maps per mesh")
        maps, table = [], np.zeros((Bn, 5), np.int64)
        for b, ft in enumerate(fts_list):
            if not isinstance(ft, torch.Tensor):
                ft = torch.as_tensor(np.asarray(ft))
            if ft.dim() != 4 or ft.shape[0] != m["n_views"][b]:
                raise ValueError(f"lift_features: mesh {b}: feature maps must be ({m['n_views'][b]}, C, H, W)")
            if ft.dtype not in (torch.float16, torch.float32):
                ft = ft.to(torch.float32)
            if ft.device != self.device:
                ft = ft.to(self.device)
            if b and (ft.dtype != maps[0].dtype or tuple(ft.shape[1:]) != tuple(maps[0].shape[1:])):
                raise ValueError("lift_features: the meshes of a call share C, H, W and the dtype of their maps")
            if any(s < 0 for s in ft.stride()):
                ft = ft.contiguous()
            maps.append(ft)
            table[b] = (ft.data_ptr(),) + tuple(ft.stride())
        self._check_stream()
        _, Cw, H, W = maps[0].shape
        proj, p2f, vis = self._lift_raster(m, H, W, focal_length, pix2face_list, "lift_features")
        table_d = self._dev(table, torch.int64, "maps")
        N = m["N"]
        out = torch.empty((Bn, N, Cw), dtype=torch.float32, device=self.device)
        cnt = torch.empty((Bn, N), dtype=torch.int32, device=self.device) if return_counts else None
        self._chk(self.lib.dm_lift_features(self.ctx, Bn, N, m["Vw"], Cw, H, W, _lib.DM_F16 if maps[0].dtype == torch.float16 else _lib.DM_F32,
                                            _ptr(table_d), _ptr(proj), _ptr(vis), _ptr(m["nv"]), _ptr(m["nw"]), _ptr(out), Cw, _ptr(cnt)))
        feats = [out[b, :n] for b, n in enumerate(m["n_verts"])]
        return (feats, [cnt[b, :n] for b, n in enumerate(m["n_verts"])]) if return_counts else feats
