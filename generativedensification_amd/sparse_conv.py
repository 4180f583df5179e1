"""Submanifold sparse 3-D convolution on the MI355X (csrc/subm_conv.hip, include/gdr.h gdr_subm_*): the one `spconv` layer
the reference's point decoder builds — `spconv.SubMConv3d(C, C, kernel_size=3, bias=True, indice_key=...)` at the head of
every Block (lightning/point_decoder/autoencoder.py) on the `SparseConvTensor` that `Point.sparsify` makes
(lightning/point_decoder/utils/structure.py).  The `spconv` package of this repository re-exports these classes.  The
semantics are restated in the header of csrc/subm_conv.hip.

GPU tensors only (no CPU fallback); anything outside the envelope raises before a kernel is launched: stride, dilation and
groups 1, odd kernel sizes 1, 3 or 5 per axis, channel counts that are multiples of 8 up to 512, fp16 / bf16 / fp32.

Sites that share a voxel (upstream leaves the winner of its hash insert to chance): every lookup answers the lowest point
index of the voxel, so such sites get identical output rows and the gradient of a non-representative site's features is zero.

Dtype rule: under autocast the features, weight and bias are cast to fp16 and the result is fp16 (spconv 2.x's
`custom_fwd(cast_inputs=torch.float16)`; INTEGRATION.md §10 lists this as an assumed convention, `AUTOCAST_DTYPE` is the
switch).  Outside autocast the computation and the result use the features' dtype.  The weight and bias gradients come back
in the parameters' dtypes.  Nothing here synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import nn

from . import _lib as L
from . import _marshal as M

__all__ = ["SparseConvTensor", "SubMConv3d", "SparseModule", "SubMTable", "build_table", "subm_conv3d", "is_spconv_module",
           "AUTOCAST_DTYPE", "TABLES_BUILT"]

AUTOCAST_DTYPE = torch.float16     # what the layer computes in under autocast (None: the features' dtype, as outside autocast)
TABLES_BUILT = 0                   # neighbour tables built by this process (tests: two layers of one indice_key build one)
_DTYPES = M.DTYPES


def _triple(v, what):
    if isinstance(v, int):
        v = (v, v, v)
    v = tuple(int(x) for x in v)
    if len(v) != 3:
        raise ValueError(f"{what} must be an int or three ints, got {v}")
    return v


class SubMTable:
    """Neighbour table of one (coordinates, kernel size): nbr (K, N) int32, rep (N) int32, order (N) int32."""

    def __init__(self, nbr, rep, order, ksize):
        self.nbr, self.rep, self.order, self.ksize = nbr, rep, order, tuple(ksize)

    def __iter__(self):      # (nbr, rep, kernel size)
        return iter((self.nbr, self.rep, self.ksize))


@torch.no_grad()
def build_table(indices, spatial_shape, batch_size, kernel_size) -> SubMTable:
    """indices (N, 4) int32 (batch, c0, c1, c2) on the GPU -> the table of include/gdr.h gdr_subm_build_table."""
    global TABLES_BUILT
    ksize = _triple(kernel_size, "kernel_size")
    if any(k not in (1, 3, 5) for k in ksize):
        raise NotImplementedError(f"kernel sizes 1, 3 and 5 per axis only, got {ksize}")
    if not isinstance(indices, torch.Tensor) or indices.dim() != 2 or indices.shape[1] != 4 or indices.dtype != torch.int32:
        raise ValueError("indices must be an (N, 4) int32 tensor of (batch, c0, c1, c2)")
    if not indices.is_cuda:
        raise RuntimeError("the HIP sparse convolution runs on ROCm/HIP tensors only (no CPU fallback)")
    shape = _triple(spatial_shape, "spatial_shape")
    N, K, dev = indices.shape[0], ksize[0] * ksize[1] * ksize[2], indices.device
    if N > L.GDR_SUBM_MAX_POINTS:
        raise ValueError(f"more than {L.GDR_SUBM_MAX_POINTS} sites")
    indices = indices.contiguous()
    lib = L.load()
    with torch.cuda.device(dev):
        nbr = torch.empty(K, N, dtype=torch.int32, device=dev)
        rep = torch.empty(N, dtype=torch.int32, device=dev)
        order = torch.empty(N, dtype=torch.int32, device=dev)
        nbytes = lib.gdr_subm_table_bytes(N)
        if nbytes == 0:
            L.check(-1, "gdr_subm_table_bytes")
        ws, base, usable = M.workspace(nbytes, dev)
        L.check(lib.gdr_subm_build_table(indices.data_ptr(), N, (C.c_int32 * 3)(*shape), int(batch_size), (C.c_int32 * 3)(*ksize),
                                         base, usable, nbr.data_ptr(), rep.data_ptr(), order.data_ptr(), M.stream()),
                "gdr_subm_build_table")
    TABLES_BUILT += 1
    return SubMTable(nbr, rep, order, ksize)


def _args(N, Cin, Cout, K, dtype) -> L.GdrSubmArgs:
    a = L.GdrSubmArgs()
    a.N, a.Cin, a.Cout, a.K, a.dtype = N, Cin, Cout, K, _DTYPES[dtype]
    return a


class _SubMConvFunction(torch.autograd.Function):
    """features (N, Cin), weight (Cout, k0, k1, k2, Cin), bias (Cout) or None, in their own dtypes; the casts to the
    computation's dtype happen in here, so that autograd hands every gradient back in its input's dtype without a detour
    through a 16-bit copy of the parameter."""

    @staticmethod
    def forward(ctx, features, weight, bias, table, dtype):
        lib = L.load()
        f = features.to(dtype)
        if f.shape[0] > 0 and f.stride(1) != 1:
            f = f.contiguous()
        w = weight.to(dtype).contiguous()
        b = None if bias is None else bias.to(dtype).contiguous()
        N, Cin = f.shape
        Cout, K, dev = w.shape[0], table.nbr.shape[0], f.device
        a = _args(N, Cin, Cout, K, dtype)
        with torch.cuda.device(dev):
            out = torch.empty(N, Cout, dtype=dtype, device=dev)
            L.check(lib.gdr_subm_conv_forward(C.byref(a), f.data_ptr(), f.stride(0) if N else Cin, table.nbr.data_ptr(),
                                              w.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(), M.stream()),
                    "gdr_subm_conv_forward")
        if any(ctx.needs_input_grad[:3]):      # (nothing is kept under no_grad)
            ctx.save_for_backward(f if ctx.needs_input_grad[1] else None, w if ctx.needs_input_grad[0] else None)
            ctx.table, ctx.a, ctx.dtype = table, a, dtype
            ctx.w_dtype, ctx.b_dtype = weight.dtype, None if bias is None else bias.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = L.load()
        f, w = ctx.saved_tensors
        a, table, dtype, dev = ctx.a, ctx.table, ctx.dtype, grad_out.device
        want_f, want_w, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_out = grad_out.to(dtype).contiguous()
        gf = gw = gb = None
        with torch.cuda.device(dev):
            if want_f:
                gf = torch.empty(a.N, a.Cin, dtype=dtype, device=dev)
            if want_w:
                gw = torch.empty(a.Cout, a.K, a.Cin, dtype=torch.float32, device=dev)
            if want_b:
                gb = torch.empty(a.Cout, dtype=torch.float32, device=dev)
            if a.N == 0:
                for t in (gw, gb):
                    if t is not None:
                        t.zero_()
            else:
                nbytes = lib.gdr_subm_backward_bytes(C.byref(a))
                if nbytes == 0:
                    L.check(-1, "gdr_subm_backward_bytes")
                ws, base, usable = M.workspace(nbytes, dev)
                L.check(lib.gdr_subm_conv_backward(
                    C.byref(a), grad_out.data_ptr(), None if f is None else f.data_ptr(), 0 if f is None else f.stride(0),
                    table.nbr.data_ptr(), table.rep.data_ptr(), table.order.data_ptr(), None if w is None else w.data_ptr(), base,
                    usable, None if gf is None else gf.data_ptr(), None if gw is None else gw.data_ptr(),
                    None if gb is None else gb.data_ptr(), M.stream()), "gdr_subm_conv_backward")
        if gw is not None:
            gw = gw.view(a.Cout, *table.ksize, a.Cin).to(ctx.w_dtype)
        if gb is not None:
            gb = gb.to(ctx.b_dtype)
        return gf, gw, gb, None, None


def subm_conv3d(features, table, weight, bias=None):
    """out[i] = bias + sum_k features[nbr[k, i]] @ W[k] (cross-correlation over the table's taps), differentiable in
    features, weight and bias.  features (N, Cin); weight (Cout, k0, k1, k2, Cin); bias (Cout) or None."""
    if not isinstance(table, SubMTable):
        raise TypeError("table must come from build_table")
    if not features.is_cuda or not weight.is_cuda:
        raise RuntimeError("the HIP sparse convolution runs on ROCm/HIP tensors only (no CPU fallback)")
    if features.dim() != 2 or weight.dim() != 5 or tuple(weight.shape[1:4]) != table.ksize or weight.shape[4] != features.shape[1]:
        raise ValueError(f"features {tuple(features.shape)} / weight {tuple(weight.shape)} do not fit kernel size {table.ksize}")
    if features.shape[0] != table.nbr.shape[1]:
        raise ValueError(f"{features.shape[0]} feature rows for a table of {table.nbr.shape[1]} sites")
    Cin, Cout = features.shape[1], weight.shape[0]
    for c in (Cin, Cout):
        if c % 8 or not 8 <= c <= L.GDR_SUBM_MAX_CHANNELS:
            raise ValueError(f"channel counts must be multiples of 8 in 8..{L.GDR_SUBM_MAX_CHANNELS}, got {Cin} -> {Cout}")
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError(f"bias must have shape ({Cout},)")
    dtype = features.dtype
    if torch.is_autocast_enabled() and AUTOCAST_DTYPE is not None:
        dtype = AUTOCAST_DTYPE
    if dtype not in _DTYPES:
        raise RuntimeError(f"the HIP sparse convolution takes fp16, bf16 or fp32, not {dtype}")
    with torch.autocast(device_type="cuda", enabled=False):
        return _SubMConvFunction.apply(features, weight, bias, table, dtype)


class SparseConvTensor:
    """spconv's container, as far as the reference uses it: features (N, C), indices (N, 4) int32 (batch, c0, c1, c2),
    spatial_shape, batch_size; `indice_dict` maps an indice_key to its SubMTable and is shared by `replace_feature`."""

    def __init__(self, features, indices, spatial_shape, batch_size, indice_dict=None):
        if indices.dim() != 2 or indices.shape[1] != 4 or indices.dtype != torch.int32:
            raise ValueError("indices must be an (N, 4) int32 tensor of (batch, c0, c1, c2)")
        if features.dim() != 2 or features.shape[0] != indices.shape[0]:
            raise ValueError("features must be (N, C) with one row per index row")
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(s) for s in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {} if indice_dict is None else indice_dict

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.indice_dict)

    def find_indice_pair(self, key):
        return None if key is None else self.indice_dict.get(key)


class SparseModule(nn.Module):
    """spconv's marker base class: what `is_spconv_module` recognises."""


def is_spconv_module(module) -> bool:
    return isinstance(module, SparseModule)


class SubMConv3d(SparseModule):
    """spconv.SubMConv3d: weight (Cout, k, k, k, Cin) and bias, initialised as nn.Conv3d initialises its own."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, **kwargs):
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"unsupported SubMConv3d arguments: {sorted(kwargs)}")
        if _triple(stride, "stride") != (1, 1, 1) or _triple(dilation, "dilation") != (1, 1, 1) or groups != 1:
            raise NotImplementedError("SubMConv3d on HIP: stride, dilation and groups must be 1")
        self.kernel_size = _triple(kernel_size, "kernel_size")
        if any(k not in (1, 3, 5) for k in self.kernel_size):
            raise NotImplementedError(f"kernel sizes 1, 3 and 5 per axis only, got {self.kernel_size}")
        for c in (in_channels, out_channels):
            if c % 8 or not 8 <= c <= L.GDR_SUBM_MAX_CHANNELS:
                raise NotImplementedError(f"channel counts must be multiples of 8 in 8..{L.GDR_SUBM_MAX_CHANNELS}")
        self.in_channels, self.out_channels, self.indice_key = in_channels, out_channels, indice_key
        self.padding = padding         # accepted and ignored: a submanifold convolution keeps the input's sites
        self.weight = nn.Parameter(torch.empty(out_channels, *self.kernel_size, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):      # nn.Conv3d's: kaiming_uniform_(a = sqrt 5) = U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), bias the same
        fan_in = self.in_channels * self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]
        bound = 1.0 / math.sqrt(fan_in)
        nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            nn.init.uniform_(self.bias, -bound, bound)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, bias={self.bias is not None}, "
                f"indice_key={self.indice_key!r}")

    def forward(self, input: SparseConvTensor) -> SparseConvTensor:
        if not isinstance(input, SparseConvTensor):
            raise TypeError("SubMConv3d takes a SparseConvTensor")
        if not input.features.is_cuda:
            raise RuntimeError("the HIP sparse convolution runs on ROCm/HIP tensors only (no CPU fallback)")
        table = input.find_indice_pair(self.indice_key)
        if table is not None and table.ksize != self.kernel_size:
            raise ValueError(f"indice_key {self.indice_key!r} was built for kernel size {table.ksize}, not {self.kernel_size}")
        if table is None:
            table = build_table(input.indices, input.spatial_shape, input.batch_size, self.kernel_size)
            if self.indice_key is not None:
                input.indice_dict[self.indice_key] = table
        return input.replace_feature(subm_conv3d(input.features, table, self.weight, self.bias))
