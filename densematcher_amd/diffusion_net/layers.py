"""
diffusion_net.layers of the reference: the DiffusionNet network with the reference's class names, constructor arguments and
state_dict keys (a released checkpoint loads with strict=True), and two routes through its forward pass:

  torch    the reference's expressions on PyTorch, on any device and dtype, with autograd: spectral and implicit_dense diffusion,
           torch.mm(gradX, .) per mesh, the two concatenations, dropout in training mode.
  device   inference in HIP (MatchEngine.diffusion_net_forward).  A float32 module with float32 input runs dm_dnet_linear_f32,
           dm_dnet_diffuse_f32, dm_dnet_gradfeat_f32; a module after .half() (every parameter float16; each input float16 or float32)
           runs dm_dnet_linear_f16, dm_dnet_diffuse_f16, dm_dnet_gradfeat_f16 -- fp16 matrix operands, fp32 accumulation and an fp32
           residual stream -- and returns float16, as the reference's half route does.
           It needs a GPU, eval mode or dropout=False, diffusion_method="spectral", and no autograd graph to record (torch.no_grad(),
           or no input and no parameter that requires grad); otherwise RuntimeError names the condition.
           differentiable=True (with route="device", opt-in) records the autograd graph instead: a float32 module with float32 input
           runs the same three fp32 kernels as torch.autograd.Functions whose backward is dm_dnet_linear_bwd_data_f32 /
           dm_dnet_linear_bwd_weight_f32, dm_dnet_diffuse_bwd_f32, dm_dnet_gradfeat_bwd_f32 (diffusion_net/backward.py); dropout, the
           tail and the loss stay torch operations, so training mode works.  It needs a GPU, diffusion_method="spectral", float32
           parameters and inputs and k_eig <= 1024.
           compute_dtype=torch.float16 (with route="device", differentiable=True) is mixed-precision training: the parameters stay
           float32 masters, every matrix (nn.Linear.weight, A_re, A_im, A) is rounded to float16 once per call, the forward runs the
           three fp16 kernels with float32 biases, times and intermediates, and the backward dm_dnet_linear_bwd_data_f16 /
           dm_dnet_linear_bwd_weight_f16, dm_dnet_diffuse_bwd_f16, dm_dnet_gradfeat_bwd_f16: fp16 matrix operands, fp32 accumulation,
           float32 gradients for the masters.  Inputs are float32, or float16 where they do not require grad.  The route does no loss
           scaling: a gradient entry below fp16's range is lost where it is staged as a matrix operand and one beyond 65504 becomes
           infinite, so torch.amp.GradScaler is used exactly as with torch.autocast.  A module after .half() stays refused.
route="auto" takes the device route where those conditions hold and tools/dnet_forward_time.py measured it faster (AUTO_DEVICE below),
else torch; it never takes the differentiable device route (route="torch" and route="auto" ignore differentiable=).  The outputs_at / last_activation tail is the same torch code behind both.

The device route reads the operators from a PackedOperators (pack_operators): fp32 padded batches of mass, evals, evecs and the ELL rows
of gradX / gradY, built once per mesh set and passed as operators=; given the reference's tensors instead, forward packs them per call.
DiffusionNet.forward_many runs a ragged list of meshes as one batched device call.

Not built on the device: gradients of a module after .half() (fp16 parameters without masters), bf16, implicit_dense, point clouds (their operators are not built either).
"""
import torch
import torch.nn as nn

from .. import _routes
from .backward import K_MAX, run as run_differentiable
from .geometry import from_basis, to_basis

# where tools/dnet_forward_time.py measured the device route faster than the torch route on an MI355X (README.md):
# "single" = one mesh per call, "batch" = several meshes in one call; "..._half": the same for a module after .half(), against the torch
# route of that module under torch.autocast("cuda")
AUTO_DEVICE = {"single": True, "batch": True, "single_half": True, "batch_half": True}

TIME_FLOOR = 1e-8


# ---------------------------------------------------------------------------------------------------------------------
class PackedOperators:
    """fp32 padded batches of what the network reads from a set of meshes: mass (B,N), evals (B,K), evecs (B,N,K); the ELL rows of
    gradX / gradY: row_len (B,N) int32, cols (B,N,nnz) int32 ascending in a row, gx, gy (B,N,nnz); n_verts (list) and n_verts_dev
    ((B) int32 on the tensors' device, None when no mesh is padded).  Padding: unit mass, zero eigenvectors, a row of length 1 on its
    own column with value 0."""
    FIELDS = ("mass", "evals", "evecs", "row_len", "cols", "gx", "gy")

    def __init__(self, n_verts, **tensors):
        self.n_verts = [int(n) for n in n_verts]
        for key in self.FIELDS:
            setattr(self, key, tensors[key])
        N = self.mass.shape[1]
        self.n_verts_dev = None if min(self.n_verts) == N else torch.tensor(self.n_verts, dtype=torch.int32, device=self.mass.device)
        self._half = None               # half_operands(), built on first use
        self._rows_t = None             # transposed_rows(), built on first use

    @property
    def device(self):
        return self.mass.device

    def to(self, device):
        """the pack on another device; its half_operands() are built there anew"""
        return PackedOperators(self.n_verts, **{key: getattr(self, key).to(device) for key in self.FIELDS})

    def half_operands(self):
        """(evecs_h, mevecs_h, e1, e2), the matrix operands of the fp16 diffusion (dm_dnet_diffuse_f16), built once on the pack's device:
        evecs_h = fp16(2^e1[b] evecs) and mevecs_h = fp16(2^e2[b] mass * evecs), (B,N,K) float16, each rounded once from the exact
        float64 value; e1, e2 (B) int32, per mesh the exponents that put the operand's largest magnitude in [2^14, 2^15) (0 for an
        operand of zeros).  Rows behind a mesh's count hold zeros."""
        if self._half is None:
            real = torch.arange(self.mass.shape[1], device=self.device)[None, :] < torch.tensor(self.n_verts, device=self.device)[:, None]
            evecs = torch.where(real[:, :, None], self.evecs.to(torch.float64), 0.0)
            mevecs = self.mass.to(torch.float64)[:, :, None] * evecs                   # 24 x 24 bits: exact
            e1, e2 = _window_exponent(evecs), _window_exponent(mevecs)
            two_to = lambda e: ((e.to(torch.int64) + 1023) << 52).view(torch.float64)   # 2^e from its bit pattern: exact
            up = lambda a, e: _round_to_half(a * two_to(e)[:, None, None])
            self._half = (up(evecs, e1), up(mevecs, e2), e1, e2)
        return self._half

    def transposed_rows(self):
        """(row_len_t, cols_t, gx_t, gy_t), the ELL rows of gradX^T and gradY^T on their union pattern, built once on the pack's device
        (the backward of the gradient features gathers over them): row_len_t (B,N) int32, cols_t (B,N,nnz_t) int32 ascending in a
        row, gx_t, gy_t (B,N,nnz_t) float32, with the padding of the forward's rows (a row without entries, and every row behind
        n_verts[b]: length 1 on its own column with value 0).  No symmetry of the pattern is assumed; entries of rows or columns
        outside a mesh are dropped."""
        if self._rows_t is None:
            Bn, N, nnz = self.cols.shape
            dev = self.device
            nv = torch.tensor(self.n_verts, device=dev)[:, None, None]
            cols = self.cols.long()
            keep = ((torch.arange(nnz, device=dev)[None, None, :] < self.row_len[:, :, None]) & (torch.arange(N, device=dev)[None, :, None] < nv)
                    & (cols >= 0) & (cols < nv))
            b, i, _ = keep.nonzero(as_tuple=True)
            j, vx, vy = cols[keep], self.gx[keep], self.gy[keep]
            order = torch.argsort((b * N + j) * N + i, stable=True)          # by (mesh, transposed row, transposed column)
            b, i, j, vx, vy = b[order], i[order], j[order], vx[order], vy[order]
            row = b * N + j
            count = torch.bincount(row, minlength=Bn * N)
            slot = torch.arange(row.numel(), device=dev) - (torch.cumsum(count, 0) - count)[row]
            nnz_t = max(int(count.max()) if row.numel() else 1, 1)
            cols_t = torch.arange(N, dtype=torch.int32, device=dev)[None, :, None].repeat(Bn, 1, nnz_t)
            gx_t = torch.zeros((Bn, N, nnz_t), dtype=torch.float32, device=dev)
            gy_t = torch.zeros_like(gx_t)
            cols_t.view(Bn * N, nnz_t)[row, slot] = i.to(torch.int32)
            gx_t.view(Bn * N, nnz_t)[row, slot] = vx
            gy_t.view(Bn * N, nnz_t)[row, slot] = vy
            self._rows_t = (count.clamp(min=1).to(torch.int32).view(Bn, N), cols_t, gx_t, gy_t)
        return self._rows_t

    def dense_grad(self, b, which="gx"):
        """(n, n) dense gradX (which="gx") or gradY ("gy") of mesh b, from its ELL rows"""
        n = self.n_verts[b]
        vals, cols, rl = getattr(self, which)[b, :n], self.cols[b, :n].long(), self.row_len[b, :n]
        out = torch.zeros((n, n), dtype=vals.dtype, device=vals.device)
        keep = torch.arange(cols.shape[1], device=cols.device)[None, :] < rl[:, None]
        rows = torch.arange(n, device=cols.device)[:, None].expand_as(cols)
        out[rows[keep], cols[keep]] = vals[keep]
        return out


def _window_exponent(a):
    """per mesh of a (B,N,K) float64 batch the integer e with 2^e max |a[b]| in [2^14, 2^15), 0 where a[b] is all zeros: (B) int32"""
    top = a.abs().amax(dim=(1, 2))
    _, x = torch.frexp(top)                                                             # top = f 2^x, f in [0.5, 1)
    return torch.where(top > 0, 15 - x, torch.zeros_like(x)).to(torch.int32)


def _round_to_half(p):
    """float64 -> float16 with ONE rounding to nearest even: first to float32 with round-to-odd (the last bit records that the value was
    inexact, so the second rounding sees on which side of a tie it lies), then the usual conversion"""
    f = p.to(torch.float32)
    d, u = f.to(torch.float64), f.view(torch.int32)
    odd = torch.where(d.abs() < p.abs(), u + 1, u - 1)
    u = torch.where((d != p) & ((u & 1) == 0), odd, u)
    return u.view(torch.float32).to(torch.float16)


def _ell_from_coo(gradX, gradY, n, device):
    """the union pattern of two (n, n) sparse COO tensors as ELL rows in ascending column order: (row_len, cols, gx, gy)"""
    ix, iy = gradX.coalesce(), gradY.coalesce()
    vx, vy = ix.values().to(torch.float32), iy.values().to(torch.float32)
    idx = torch.cat((ix.indices(), iy.indices()), dim=1)
    both = torch.cat((torch.stack((vx, torch.zeros_like(vx)), 1), torch.stack((torch.zeros_like(vy), vy), 1)), 0)
    sp = torch.sparse_coo_tensor(idx, both, (n, n, 2)).coalesce()          # sorted by (row, column); v + 0 is exact
    rows, cols, vals = sp.indices()[0], sp.indices()[1], sp.values()
    row_len = torch.bincount(rows, minlength=n)
    start = torch.cumsum(row_len, 0) - row_len
    q = torch.arange(rows.numel(), device=rows.device) - start[rows]
    nnz = max(int(row_len.max()) if n else 1, 1)
    ell_cols = torch.arange(n, device=rows.device, dtype=torch.int32)[:, None].repeat(1, nnz)
    gx = torch.zeros((n, nnz), dtype=torch.float32, device=rows.device)
    gy = torch.zeros_like(gx)
    ell_cols[rows, q] = cols.to(torch.int32)
    gx[rows, q] = vals[:, 0]
    gy[rows, q] = vals[:, 1]
    empty = row_len == 0                                                     # (a row without entries: the padding convention)
    row_len = torch.where(empty, torch.ones_like(row_len), row_len).to(torch.int32)
    return row_len.to(device), ell_cols.to(device), gx.to(device), gy.to(device)


def _one_mesh(op):
    """(mass, evals, evecs, row_len, cols, gx, gy) in fp32 on the operator's own device, from a dict of MatchEngine.diffusion_operators
    or a tuple of get_operators (frames, mass, L, evals, evecs, gradX, gradY; gradX / gradY None: no gradient rows)"""
    f32 = lambda t: t.detach().to(torch.float32)
    if isinstance(op, dict):
        return (f32(op["mass"]), f32(op["evals"]), f32(op["evecs"]), op["row_len"].to(torch.int32), op["cols"].to(torch.int32),
                f32(op["gx"]), f32(op["gy"]))
    _, mass, _, evals, evecs, gradX, gradY = op
    n = mass.shape[0]
    if gradX is None or gradY is None:
        ell = (torch.ones(n, dtype=torch.int32, device=mass.device), torch.arange(n, dtype=torch.int32, device=mass.device)[:, None],
               torch.zeros((n, 1), dtype=torch.float32, device=mass.device), torch.zeros((n, 1), dtype=torch.float32, device=mass.device))
    else:
        ell = _ell_from_coo(gradX.detach(), gradY.detach(), n, gradX.device)
    return (f32(mass), f32(evals), f32(evecs)) + ell


def pack_operators(ops, device=None):
    """A reusable PackedOperators of a mesh set.  ops: a list with, per mesh, the tuple get_operators / get_all_operators return
    (the coalesced COO of gradX / gradY goes to ELL on its device, rows in ascending column) or the dict of
    MatchEngine.diffusion_operators (its device ELL as it is, rounded once to fp32); one such tuple or dict alone is a set of one.
    Meshes may differ in size (padded to the largest, n_verts recorded) but share k_eig.  device: where the pack goes (default: where
    the first mesh's operators are)."""
    if isinstance(ops, tuple) and len(ops) == 7 and isinstance(ops[1], (list, tuple)):
        ops = list(zip(*ops))                      # the seven lists of get_all_operators
    elif isinstance(ops, dict) or (isinstance(ops, tuple) and len(ops) == 7 and not isinstance(ops[1], dict)):
        ops = [ops]
    per = [_one_mesh(op) for op in ops]
    if not per:
        raise ValueError("pack_operators: no mesh")
    device = per[0][0].device if device is None else torch.device(device)
    n_verts = [p[0].shape[0] for p in per]
    Bn, N, K = len(per), max(n_verts), per[0][1].shape[0]
    if any(p[1].shape[0] != K or p[2].shape != (n, K) for p, n in zip(per, n_verts)):
        raise ValueError("pack_operators: the meshes must share k_eig, with evecs (n, k_eig) each")
    nnz = max(p[4].shape[1] for p in per)
    out = {"mass": torch.ones((Bn, N), dtype=torch.float32, device=device),
           "evals": torch.zeros((Bn, K), dtype=torch.float32, device=device),
           "evecs": torch.zeros((Bn, N, K), dtype=torch.float32, device=device),
           "row_len": torch.ones((Bn, N), dtype=torch.int32, device=device),
           "cols": torch.arange(N, dtype=torch.int32, device=device)[None, :, None].repeat(Bn, 1, nnz),
           "gx": torch.zeros((Bn, N, nnz), dtype=torch.float32, device=device),
           "gy": torch.zeros((Bn, N, nnz), dtype=torch.float32, device=device)}
    for b, (p, n) in enumerate(zip(per, n_verts)):
        mass, evals, evecs, row_len, cols, gx, gy = (t.to(device) for t in p)
        w = cols.shape[1]
        out["mass"][b, :n], out["evals"][b], out["evecs"][b, :n], out["row_len"][b, :n] = mass, evals, evecs, row_len
        out["cols"][b, :n, :w], out["gx"][b, :n, :w], out["gy"][b, :n, :w] = cols, gx, gy
    return PackedOperators(n_verts, **out)


# ---------------------------------------------------------------------------------------------------------------------
class LearnedTimeDiffusion(nn.Module):
    """Heat diffusion with one learned time per channel: spectral (exp(-evals t) in the eigenbasis) or implicit_dense (a dense solve
    with M + t L per channel).  x (B,V,C), L (B,V,V) sparse or None, mass (B,V), evals (B,K), evecs (B,V,K) -> (B,V,C)."""

    def __init__(self, C_inout, method="spectral"):
        super().__init__()
        self.C_inout = C_inout
        self.diffusion_time = nn.Parameter(torch.Tensor(C_inout))
        self.method = method
        nn.init.constant_(self.diffusion_time, 0.0)

    def clamp_time(self):
        """times stay positive: the parameter is clamped in place, as the reference leaves it after every forward"""
        with torch.no_grad():
            self.diffusion_time.data = torch.clamp(self.diffusion_time, min=TIME_FLOOR)

    def forward(self, x, L, mass, evals, evecs):
        self.clamp_time()
        if x.shape[-1] != self.C_inout:
            raise ValueError("Tensor has wrong shape = {}. Last dim shape should have number of channels = {}".format(x.shape, self.C_inout))
        if self.method == "spectral":
            x_spec = to_basis(x, evecs, mass)
            coefs = torch.exp(-evals.unsqueeze(-1) * self.diffusion_time.unsqueeze(0))
            return from_basis(coefs * x_spec, evecs)
        if self.method == "implicit_dense":
            V = x.shape[-2]
            mat = L.to_dense().unsqueeze(1).expand(-1, self.C_inout, V, V).clone()
            mat *= self.diffusion_time.unsqueeze(0).unsqueeze(-1).unsqueeze(-1)
            mat += torch.diag_embed(mass).unsqueeze(1)
            chol = torch.linalg.cholesky(mat)
            rhs = torch.transpose(x * mass.unsqueeze(-1), 1, 2).unsqueeze(-1)
            return torch.transpose(torch.cholesky_solve(rhs, chol).squeeze(-1), 1, 2)
        raise ValueError("unrecognized method")


class SpatialGradientFeatures(nn.Module):
    """tanh of the per-channel inner product of the gradient with a learned (complex-)linear image of itself:
    vectors (V,C,2) -> (V,C)"""

    def __init__(self, C_inout, with_gradient_rotations=True):
        super().__init__()
        self.C_inout = C_inout
        self.with_gradient_rotations = with_gradient_rotations
        if with_gradient_rotations:
            self.A_re = nn.Linear(C_inout, C_inout, bias=False)
            self.A_im = nn.Linear(C_inout, C_inout, bias=False)
        else:
            self.A = nn.Linear(C_inout, C_inout, bias=False)

    def forward(self, vectors):
        vx, vy = vectors[..., 0], vectors[..., 1]
        if self.with_gradient_rotations:
            b_re = self.A_re(vx) - self.A_im(vy)
            b_im = self.A_re(vy) + self.A_im(vx)
        else:
            b_re, b_im = self.A(vx), self.A(vy)
        return torch.tanh(vx * b_re + vy * b_im)


class MiniMLP(nn.Sequential):
    """Linear layers with an activation between them (none after the last) and, with dropout, a Dropout in front of every layer
    but the first"""

    def __init__(self, layer_sizes, dropout=False, activation=nn.ReLU, name="miniMLP"):
        super().__init__()
        for i in range(len(layer_sizes) - 1):
            if dropout and i > 0:
                self.add_module(name + "_mlp_layer_dropout_{:03d}".format(i), nn.Dropout(p=0.5))
            self.add_module(name + "_mlp_layer_{:03d}".format(i), nn.Linear(layer_sizes[i], layer_sizes[i + 1]))
            if i + 2 != len(layer_sizes):
                self.add_module(name + "_mlp_act_{:03d}".format(i), activation())


class DiffusionNetBlock(nn.Module):
    """diffusion -> gradient features -> MLP over (x, x_diffuse, x_grad) -> + x, at the vertices"""

    def __init__(self, C_width, mlp_hidden_dims, dropout=True, diffusion_method="spectral", with_gradient_features=True,
                 with_gradient_rotations=True):
        super().__init__()
        self.C_width = C_width
        self.mlp_hidden_dims = mlp_hidden_dims
        self.dropout = dropout
        self.with_gradient_features = with_gradient_features
        self.with_gradient_rotations = with_gradient_rotations
        self.diffusion = LearnedTimeDiffusion(C_width, method=diffusion_method)
        self.MLP_C = 2 * C_width
        if with_gradient_features:
            self.gradient_features = SpatialGradientFeatures(C_width, with_gradient_rotations=with_gradient_rotations)
            self.MLP_C += C_width
        self.mlp = MiniMLP([self.MLP_C] + list(mlp_hidden_dims) + [C_width], dropout=dropout)

    def forward(self, x_in, mass, L, evals, evecs, gradX, gradY):
        B = x_in.shape[0]
        if x_in.shape[-1] != self.C_width:
            raise ValueError("Tensor has wrong shape = {}. Last dim shape should have number of channels = {}".format(x_in.shape, self.C_width))
        x_diffuse = self.diffusion(x_in, L, mass, evals, evecs)
        feats = [x_in, x_diffuse]
        if self.with_gradient_features:
            grads = []
            with torch.autocast("cuda", enabled=False):       # torch.mm has no batched sparse form: one mesh at a time
                for b in range(B):
                    xb = x_diffuse[b, ...].float()
                    grads.append(torch.stack((torch.mm(gradX[b, ...], xb), torch.mm(gradY[b, ...], xb)), dim=-1))
            feats.append(self.gradient_features(torch.stack(grads, dim=0)))
        return self.mlp(torch.cat(feats, dim=-1)) + x_in

    def device_weights(self):
        """this block's parameters as MatchEngine.diffusion_net_forward takes them (no copies)"""
        gf = self.gradient_features if self.with_gradient_features else None
        A_re = None if gf is None else (gf.A_re.weight.data if self.with_gradient_rotations else gf.A.weight.data)
        A_im = gf.A_im.weight.data if gf is not None and self.with_gradient_rotations else None
        mlp = [(m.weight.data, m.bias.data) for m in self.mlp if isinstance(m, nn.Linear)]
        return {"times": self.diffusion.diffusion_time.data, "A_re": A_re, "A_im": A_im, "mlp": mlp}


class DiffusionNet(nn.Module):
    """The network: first_lin, N_block DiffusionNetBlocks, last_lin, then the outputs_at remap ('vertices', 'edges', 'faces',
    'global_mean') and last_activation.  Constructor arguments and parameter names are the reference's."""

    def __init__(self, C_in, C_out, C_width=128, N_block=4, last_activation=None, outputs_at="vertices", mlp_hidden_dims=None, dropout=True,
                 with_gradient_features=True, with_gradient_rotations=True, diffusion_method="spectral"):
        super().__init__()
        self.C_in, self.C_out, self.C_width, self.N_block = C_in, C_out, C_width, N_block
        self.last_activation = last_activation
        self.outputs_at = outputs_at
        if outputs_at not in ["vertices", "edges", "faces", "global_mean"]:
            raise ValueError("invalid setting for outputs_at")
        if mlp_hidden_dims is None:
            mlp_hidden_dims = [C_width, C_width]
        self.mlp_hidden_dims = mlp_hidden_dims
        self.dropout = dropout
        self.diffusion_method = diffusion_method
        if diffusion_method not in ["spectral", "implicit_dense"]:
            raise ValueError("invalid setting for diffusion_method")
        self.with_gradient_features = with_gradient_features
        self.with_gradient_rotations = with_gradient_rotations
        self.first_lin = nn.Linear(C_in, C_width)
        self.last_lin = nn.Linear(C_width, C_out)
        self.blocks = []
        for i_block in range(N_block):
            block = DiffusionNetBlock(C_width=C_width, mlp_hidden_dims=mlp_hidden_dims, dropout=dropout, diffusion_method=diffusion_method,
                                      with_gradient_features=with_gradient_features, with_gradient_rotations=with_gradient_rotations)
            self.blocks.append(block)
            self.add_module("block_" + str(i_block), block)
        self.last_route = None          # the route the last forward took ("torch" or "device")

    # ------------------------------------------------------------------ routes
    def _device_obstacle(self, xs, extra=(), differentiable=False, k_eig=None, mixed=False):
        """None when the device route can run for these inputs, else the condition that keeps it from running.  differentiable: the
        route that records the autograd graph (training mode and tensors that require grad are no obstacles; float32 only).  mixed:
        its fp16 family (compute_dtype=torch.float16): float32 parameters; inputs float32, or float16 where they do not require grad"""
        if not torch.cuda.is_available():
            return "it needs a ROCm GPU (gfx950)"
        if any(not x.is_cuda for x in xs):
            return "the input must be on the GPU"
        if self.diffusion_method != "spectral":
            return "diffusion_method must be 'spectral' (implicit_dense is not built on the device)"
        if self.training and self.dropout and not differentiable:
            return "the module must be in eval mode or built with dropout=False"
        params = list(self.parameters())
        if differentiable and any(t.dtype != torch.float32 for t in (params if mixed else list(xs) + params)):
            return "the parameters and inputs must be float32 (the fp16 kernels have no backward)"
        why = self._mixed_input_obstacle(xs) if differentiable and mixed else self._dtype_obstacle(xs)
        if why is not None:
            return why
        if any(not p.is_cuda for p in params):
            return "the parameters must be on the GPU"
        if differentiable:
            return None if k_eig is None or k_eig <= K_MAX else "k_eig must be at most {} (the diffusion kernels' limit), not {}".format(K_MAX, k_eig)
        return _routes.grad_obstacle(list(xs) + params + [t for t in extra if isinstance(t, torch.Tensor)])

    def _dtype_obstacle(self, xs):
        """None for a float32 module with float32 inputs or a float16 module with float16 / float32 inputs, else what is wrong"""
        kinds = {p.dtype for p in self.parameters()}
        if kinds == {torch.float32}:
            return None if all(x.dtype == torch.float32 for x in xs) else "the input and the parameters must be float32"
        if kinds == {torch.float16}:
            return None if all(x.dtype in (torch.float16, torch.float32) for x in xs) else "with float16 parameters every input must be float16 or float32"
        return "the parameters must be all float32 or all float16, not " + ", ".join(sorted(str(k)[6:] for k in kinds))

    @staticmethod
    def _mixed_input_obstacle(xs):
        """compute_dtype=torch.float16: None for float32 inputs and float16 inputs that do not require grad, else what is wrong"""
        for x in xs:
            if x.dtype not in (torch.float16, torch.float32):
                return "with compute_dtype=torch.float16 every input must be float32 or float16, not " + str(x.dtype)[6:]
            if x.dtype == torch.float16 and x.requires_grad:
                return "with compute_dtype=torch.float16 a float16 input must not require grad (the input gradient is float32)"
        return None

    @staticmethod
    def _mixed(compute_dtype):
        """whether compute_dtype asks for the fp16 family of the differentiable device route; ValueError for what it cannot be"""
        if compute_dtype is not None and compute_dtype != torch.float16:
            raise ValueError("compute_dtype must be None or torch.float16, not {}".format(compute_dtype))
        return compute_dtype is not None

    def is_half(self):
        return self.first_lin.weight.dtype == torch.float16

    def _tail(self, x, mass, edges, faces):
        if self.outputs_at == "vertices":
            x_out = x
        elif self.outputs_at == "edges":
            x_gather = x.unsqueeze(-1).expand(-1, -1, -1, 2)
            x_out = torch.mean(torch.gather(x_gather, 1, edges.unsqueeze(2).expand(-1, -1, x.shape[-1], -1)), dim=-1)
        elif self.outputs_at == "faces":
            x_gather = x.unsqueeze(-1).expand(-1, -1, -1, 3)
            x_out = torch.mean(torch.gather(x_gather, 1, faces.unsqueeze(2).expand(-1, -1, x.shape[-1], -1)), dim=-1)
        else:       # the mass-weighted mean over the vertices
            x_out = torch.sum(x * mass.unsqueeze(-1), dim=-2) / torch.sum(mass, dim=-1, keepdim=True)
        if self.last_activation is not None:
            x_out = self.last_activation(x_out)
        return x_out

    def device_weights(self):
        for b in self.blocks:
            b.diffusion.clamp_time()
        return {"first": (self.first_lin.weight.data, self.first_lin.bias.data), "last": (self.last_lin.weight.data, self.last_lin.bias.data),
                "blocks": [b.device_weights() for b in self.blocks]}

    def _run_device(self, xs, packed, differentiable=False, mixed=False):
        from ..engine import default_engine
        eng = default_engine(xs[0].device)
        if packed.device != eng.device:
            packed = packed.to(eng.device)
        if differentiable:
            return run_differentiable(self, eng, xs, packed, half=mixed)
        with torch.no_grad():
            return eng.diffusion_net_forward(self.device_weights(), packed, xs if len(xs) > 1 else xs[0])

    def forward(self, x_in, mass=None, L=None, evals=None, evecs=None, gradX=None, gradY=None, edges=None, faces=None, *, route="auto", operators=None,
                differentiable=False, compute_dtype=None):
        """x_in (N,C_in) or (B,N,C_in), or a tuple of up to three such tensors read as concatenated along the channels; mass (N) / (B,N),
        L, evals (K), evecs (N,K), gradX, gradY sparse (N,N) (or with the batch dimension), edges / faces for outputs_at.
        operators: a PackedOperators of the B meshes (device route; mass may then be None).  differentiable: with route="device", record
        the autograd graph through the backward kernels (module docstring); ignored by route="torch" and route="auto".
        compute_dtype: None, or torch.float16 -- with route="device", differentiable=True the mixed-precision family (float32 master
        parameters, fp16 matrix operands, float32 gradients; no loss scaling of its own: use torch.amp.GradScaler as with
        torch.autocast); ignored like differentiable=; any other dtype is a ValueError.  Returns (N,C_out) or (B,N,C_out), or what
        outputs_at makes of it."""
        xs = list(x_in) if isinstance(x_in, (tuple, list)) else [x_in]
        if not 1 <= len(xs) <= 3:
            raise ValueError("x_in: one tensor or a tuple of up to three")
        if sum(x.shape[-1] for x in xs) != self.C_in:
            raise ValueError("DiffusionNet was constructed with C_in={}, but x_in has last dim={}".format(self.C_in, sum(x.shape[-1] for x in xs)))
        if xs[0].dim() not in (2, 3):
            raise ValueError("x_in should be tensor with shape [N,C] or [B,N,C]")
        flat = xs[0].dim() == 2
        if flat:
            up = lambda t: None if t is None else t.unsqueeze(0)
            xs = [x.unsqueeze(0) for x in xs]
            mass, L, evals, evecs, gradX, gradY, edges, faces = (up(t) for t in (mass, L, evals, evecs, gradX, gradY, edges, faces))
        differentiable = bool(differentiable) and route == "device"
        mixed = self._mixed(compute_dtype) and differentiable
        k_eig = operators.evals.shape[-1] if operators is not None else (None if evals is None else evals.shape[-1])
        picked = _routes.pick_torch(route, "DiffusionNet", lambda: self._device_obstacle(xs, (mass, evals, evecs), differentiable, k_eig, mixed),
                                    AUTO_DEVICE[("batch" if xs[0].shape[0] > 1 else "single") + ("_half" if self.is_half() else "")], refusal=RuntimeError)
        self.last_route = picked
        if picked == "torch":
            if mass is None or (self.diffusion_method == "spectral" and (evals is None or evecs is None)):
                raise ValueError("route='torch' takes the reference's tensors (mass, evals, evecs, gradX, gradY), not a PackedOperators alone")
            x = self.first_lin(xs[0] if len(xs) == 1 else torch.cat(xs, dim=-1))
            for b in self.blocks:
                x = b(x, mass, L, evals, evecs, gradX, gradY)
            x = self.last_lin(x)
        else:
            packed = operators
            if packed is None:
                Bn = xs[0].shape[0]
                need = self.with_gradient_features
                packed = pack_operators([(None, mass[b], None, evals[b], evecs[b], gradX[b] if need else None, gradY[b] if need else None)
                                         for b in range(Bn)], device=xs[0].device)
            if len(packed.n_verts) != xs[0].shape[0] or packed.mass.shape[1] != xs[0].shape[1]:
                raise ValueError("operators: packed for {} meshes of up to {} vertices, x_in is {}".format(len(packed.n_verts), packed.mass.shape[1], tuple(xs[0].shape)))
            x = self._run_device(xs, packed, differentiable, mixed)
            if mass is None:
                mass = packed.mass
        x_out = self._tail(x, mass, edges, faces)
        return x_out.squeeze(0) if flat else x_out

    def forward_many(self, x_list, packed, edges=None, faces=None, differentiable=False, compute_dtype=None):
        """A ragged list of meshes as ONE batched device call: x_list[b] (n_b, C_in), or a tuple of up to three such tensors per mesh;
        packed: the PackedOperators of the same meshes.  Returns the list of outputs, each what forward() returns for its mesh alone
        (edges / faces: lists, for outputs_at).  differentiable, compute_dtype: as in forward with route="device"."""
        per = [list(x) if isinstance(x, (tuple, list)) else [x] for x in x_list]
        if len(per) != len(packed.n_verts) or any(p[0].shape[0] != n for p, n in zip(per, packed.n_verts)):
            raise ValueError("forward_many: x_list does not match the packed meshes")
        mixed = self._mixed(compute_dtype) and bool(differentiable)
        why = self._device_obstacle([x for p in per for x in p], (), bool(differentiable), packed.evals.shape[-1], mixed)
        if why is not None:
            raise RuntimeError("DiffusionNet.forward_many: " + why)
        self.last_route = "device"
        Bn, N = len(per), packed.mass.shape[1]
        xs = []
        for s in range(len(per[0])):
            buf = torch.zeros((Bn, N, per[0][s].shape[-1]), dtype=per[0][s].dtype, device=per[0][s].device)
            for b, p in enumerate(per):
                buf[b, :p[s].shape[0]] = p[s]
            xs.append(buf)
        if sum(x.shape[-1] for x in xs) != self.C_in:
            raise ValueError("DiffusionNet was constructed with C_in={}, but x_list has last dim={}".format(self.C_in, sum(x.shape[-1] for x in xs)))
        x = self._run_device(xs, packed, bool(differentiable), mixed)
        mass = packed.mass.to(x.device)
        return [self._tail(x[b:b + 1, :n], mass[b:b + 1, :n], None if edges is None else edges[b].unsqueeze(0),
                           None if faces is None else faces[b].unsqueeze(0)).squeeze(0) for b, n in enumerate(packed.n_verts)]
