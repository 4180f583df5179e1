"""CSR segment reductions for the point decoder on the MI355X (csrc/segment.hip, include/gdr.h gdr_seg_*): the functions the
reference's lightning/point_decoder takes from `torch_scatter` (segment_csr, gather_csr, scatter_mean, scatter_std, ...) and
from `torch_geometric.utils` (scatter, softmax, cumsum), with their names, argument order and keyword names.  The packages
`torch_scatter` and `torch_geometric` at the root of this repository re-export them.

GPU tensors only (no CPU fallback: a CPU tensor raises RuntimeError).  The envelope is what the reference calls:
  * segment_csr / gather_csr: a 1-D `indptr`, reduction along dim 0, trailing dimensions of `src` flattened into channels;
    a batched indptr raises NotImplementedError;
  * scatter*: dim 0 (or -src.dim()), `index` 1-D or a broadcast of a 1-D index along dim 0; anything else raises
    NotImplementedError.  The index is ALWAYS stable-sorted (gdr_serial_sort), then the CSR kernels run with the permutation;
  * f32, f16, bf16 (f32 accumulation, result in the source dtype; no autocast rule: a call computes in the dtype it is
    given); int64 for sum and gather.  Other dtypes raise TypeError.

Conventions (restated from the packages' documentation): an empty segment gives 0 for every reduction and
arg = N; mean divides by max(count, 1); min / max report the lowest row among ties and the gradient goes to that row alone;
scatter_std = sqrt(sum_sq / (clamp(count - 1, 1) + 1e-6)) (unbiased) around the per-segment mean; softmax divides by
(sum + 1e-16).  Nothing synchronises with the host except `dim_size=None` / `num_nodes=None` with an index (one read of
index.max()) and `gather_csr` without `out` (one read of indptr[-1], the number of output rows), both as upstream.  No
atomics: every call is bitwise reproducible.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["segment_csr", "segment_sum_csr", "segment_mean_csr", "segment_min_csr", "segment_max_csr", "gather_csr", "scatter",
           "scatter_sum", "scatter_add", "scatter_mean", "scatter_min", "scatter_max", "scatter_std", "softmax", "cumsum"]

ROWS = L.GDR_SEG_ROWS     # rows per run of the kernels (the chunk R of DESIGN §17)

_DTYPES = {**M.DTYPES, torch.int64: L.GDR_SEG_DTYPES["i64"]}
_NO_CPU = "the HIP segment reductions run on ROCm/HIP tensors only (no CPU fallback)"


# ---- argument checks ------------------------------------------------------------------------------------------------------

def _check_src(src):
    if not isinstance(src, torch.Tensor):
        raise TypeError(f"src must be a tensor, not {type(src).__name__}")
    if not src.is_cuda:
        raise RuntimeError(_NO_CPU)
    if src.dim() < 1:
        raise ValueError("src must have at least one dimension")
    if src.dtype not in _DTYPES:
        raise TypeError(f"src must be float32, float16, bfloat16 or int64, not {src.dtype}")


def _check_ptr_layout(indptr):
    if not isinstance(indptr, torch.Tensor):
        raise TypeError(f"indptr must be a tensor, not {type(indptr).__name__}")
    if indptr.dim() != 1:
        raise NotImplementedError("only a 1-D indptr (reduction along dim 0) is supported; a batched indptr is not")


def _check_ptr(indptr, src):
    if not indptr.is_cuda or indptr.device != src.device:
        raise RuntimeError(_NO_CPU if not indptr.is_cuda else "indptr must live on src's device")
    if indptr.dtype.is_floating_point or indptr.dtype.is_complex or indptr.dtype == torch.bool:
        raise TypeError(f"indptr must be an integer tensor, not {indptr.dtype}")
    if indptr.numel() < 1:
        raise ValueError("indptr needs at least one entry")
    return indptr.long().contiguous()


def _rows(src):
    """src (N, ...) as an (N, C) view whose channels are unit-stride, C >= 1 (a copy only where the layout forces one)."""
    n = src.shape[0]
    c = src.numel() // n if n else int(torch.Size(src.shape[1:]).numel())
    x = src.reshape(n, c)
    if c > 1 and x.stride(1) != 1 or (n > 1 and x.stride(0) < c):
        x = x.contiguous()
    return x


def _stride0(x):
    return x.stride(0) if x.shape[0] > 1 else max(x.shape[1], 1)


# ---- the four primitives --------------------------------------------------------------------------------------------------

def _reduce(x, perm, indptr, op):
    """x (N, C), perm None or (N) int64, indptr (S + 1) int64 -> out (S, C) and, for min / max, arg (S, C) int64."""
    N, C = x.shape
    S = indptr.numel() - 1
    dev = x.device
    if x.dtype == torch.int64 and op != "sum":
        raise TypeError(f"int64 is supported for reduce='sum' only, not {op!r}")
    with torch.cuda.device(dev):
        out = torch.empty(S, C, dtype=x.dtype, device=dev)
        arg = torch.empty(S, C, dtype=torch.int64, device=dev) if op in ("min", "max") else None
        if S == 0 or C == 0:
            return out, arg
        lib = L.load()
        nbytes = lib.gdr_seg_reduce_bytes(N, S, C)
        if nbytes == 0:
            L.check(-1, "gdr_seg_reduce_bytes")
        ws, base, usable = M.workspace(nbytes, dev)
        L.check(lib.gdr_seg_reduce(M.ptr_or_none_if_empty(x), _stride0(x), M.ptr(perm), indptr.data_ptr(), N, S, C,
                                   _DTYPES[x.dtype], L.GDR_SEG_OPS[op], base, usable, out.data_ptr(), M.ptr(arg), M.stream()),
                "gdr_seg_reduce")
    return out, arg


def _gather(x, perm, indptr, N, inv_count=False, fill_outside=False, out=None):
    """x (S, C) -> (N, C): row perm[r] (or r) = x[segment of r]; `out` given: written in place where a segment covers it."""
    S, C = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(N, C, dtype=x.dtype, device=dev)
        if N == 0 or C == 0:
            return out
        L.check(L.load().gdr_seg_gather(M.ptr_or_none_if_empty(x), _stride0(x), indptr.data_ptr(), M.ptr(perm), N, S, C,
                                        _DTYPES[x.dtype], int(inv_count), int(fill_outside), out.data_ptr(), M.stream()),
                "gdr_seg_gather")
    return out


def _route(grad_out, arg, N):
    S, C = grad_out.shape
    dev = grad_out.device
    with torch.cuda.device(dev):
        grad_src = torch.empty(N, C, dtype=grad_out.dtype, device=dev)
        if N == 0 or C == 0:
            return grad_src
        L.check(L.load().gdr_seg_route(M.ptr_or_none_if_empty(grad_out), M.ptr_or_none_if_empty(arg), N, S, C,
                                       _DTYPES[grad_out.dtype], grad_src.data_ptr(), M.stream()), "gdr_seg_route")
    return grad_src


def _sorted_route(index, S):
    """index (N) int64 -> (perm, indptr): the stable argsort of the index and the CSR pointer of its S segments."""
    N, dev = index.numel(), index.device
    lib = L.load()
    with torch.cuda.device(dev):
        perm = torch.empty(N, dtype=torch.int64, device=dev)
        indptr = torch.empty(S + 1, dtype=torch.int64, device=dev)
        if N:
            inverse = torch.empty(1, N, dtype=torch.int64, device=dev)
            nbytes = lib.gdr_serial_sort_bytes(1, N)
            if nbytes == 0:
                L.check(-1, "gdr_serial_sort_bytes")
            ws, base, usable = M.workspace(nbytes, dev)
            bits = max(1, (max(S, 1) - 1).bit_length())
            L.check(lib.gdr_serial_sort(index.data_ptr(), 1, N, bits, base, usable, perm.data_ptr(), inverse.data_ptr(),
                                        M.stream()), "gdr_serial_sort")
        L.check(lib.gdr_seg_ptr_from_sorted(M.ptr_or_none_if_empty(index), M.ptr_or_none_if_empty(perm), N, S,
                                            indptr.data_ptr(), M.stream()), "gdr_seg_ptr_from_sorted")
    return perm, indptr


# ---- autograd -------------------------------------------------------------------------------------------------------------

class _Reduce(torch.autograd.Function):
    """(src, perm or None, indptr, op) -> out, arg (arg: an empty int64 tensor for sum / mean)"""

    @staticmethod
    def forward(ctx, src, perm, indptr, op):
        x = _rows(src)
        out, arg = _reduce(x, perm, indptr, op)
        ctx.op, ctx.shape = op, src.shape
        ctx.save_for_backward(perm, indptr, arg)
        shape = (indptr.numel() - 1,) + tuple(src.shape[1:])
        if arg is None:
            arg_out = torch.empty(0, dtype=torch.int64, device=src.device)
        else:
            arg_out = arg.view(shape)
        ctx.mark_non_differentiable(arg_out)
        return out.view(shape), arg_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_arg):
        perm, indptr, arg = ctx.saved_tensors
        N = ctx.shape[0]
        g = _rows(grad_out)
        if ctx.op in ("sum", "mean"):
            grad = _gather(g, perm, indptr, N, inv_count=ctx.op == "mean", fill_outside=True)
        else:
            grad = _route(g.contiguous(), arg, N)
        return grad.view(ctx.shape), None, None, None


class _Gather(torch.autograd.Function):
    """(src (S, ...), perm or None, indptr, N) -> (N, ...); rows in no segment are zero"""

    @staticmethod
    def forward(ctx, src, perm, indptr, N):
        x = _rows(src)
        ctx.shape = src.shape
        ctx.save_for_backward(perm, indptr)
        return _gather(x, perm, indptr, N, fill_outside=True).view((N,) + tuple(src.shape[1:]))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        perm, indptr = ctx.saved_tensors
        grad, _ = _reduce(_rows(grad_out), perm, indptr, "sum")
        return grad.view(ctx.shape), None, None, None


class _Softmax(torch.autograd.Function):
    """(src (N, ...), perm or None, indptr) -> softmax over the rows of every segment, per channel"""

    @staticmethod
    def forward(ctx, src, perm, indptr):
        x = _rows(src)
        N = x.shape[0]
        seg_max, _ = _reduce(x, perm, indptr, "max")
        e = torch.exp(x - _gather(seg_max, perm, indptr, N, fill_outside=True))
        seg_sum, _ = _reduce(e, perm, indptr, "sum")
        y = e / (_gather(seg_sum, perm, indptr, N, fill_outside=True) + 1e-16)
        if perm is None:      # a pointer need not cover every row: rows outside [ptr[0], ptr[-1]) get 0 (and no gradient)
            y = y * _gather(torch.ones(seg_sum.shape[0], 1, dtype=x.dtype, device=x.device), None, indptr, N, fill_outside=True)
        ctx.save_for_backward(perm, indptr, y)
        return y.view(src.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        perm, indptr, y = ctx.saved_tensors
        g = _rows(grad_out)
        dot, _ = _reduce(g * y, perm, indptr, "sum")
        grad = y * (g - _gather(dot, perm, indptr, y.shape[0], fill_outside=True))
        return grad.view(grad_out.shape), None, None


def _finish(res, out):
    if out is None:
        return res
    out.copy_(res)
    return out


# ---- torch_scatter: CSR ---------------------------------------------------------------------------------------------------

def _segment(src, indptr, out, op):
    _check_ptr_layout(indptr)       # (what is not supported is said before where it would run)
    _check_src(src)
    indptr = _check_ptr(indptr, src)
    res, arg = _Reduce.apply(src, None, indptr, op)
    return _finish(res, out), arg


def segment_sum_csr(src, indptr, out=None):
    return _segment(src, indptr, out, "sum")[0]


def segment_mean_csr(src, indptr, out=None):
    return _segment(src, indptr, out, "mean")[0]


def segment_min_csr(src, indptr, out=None):
    return _segment(src, indptr, out, "min")


def segment_max_csr(src, indptr, out=None):
    return _segment(src, indptr, out, "max")


def segment_csr(src, indptr, out=None, reduce="sum"):
    """out[s] = reduce over src[indptr[s] : indptr[s + 1]] along dim 0; reduce: sum / add / mean / min / max."""
    if reduce == "add":
        reduce = "sum"
    if reduce not in L.GDR_SEG_OPS:
        raise ValueError(f"reduce must be one of sum, add, mean, min, max; got {reduce!r}")
    return _segment(src, indptr, out, reduce)[0]


def gather_csr(src, indptr, out=None):
    """out[i] = src[s] for indptr[s] <= i < indptr[s + 1]; without `out` the result has indptr[-1] rows (one read-back),
    with `out` only the rows a segment covers are written (and the call is not recorded for autograd)."""
    _check_ptr_layout(indptr)
    _check_src(src)
    indptr = _check_ptr(indptr, src)
    if src.shape[0] != indptr.numel() - 1:
        raise ValueError(f"src has {src.shape[0]} rows for {indptr.numel() - 1} segments")
    if out is not None:
        if not out.is_cuda:
            raise RuntimeError(_NO_CPU)
        if out.dtype != src.dtype or out.shape[1:] != src.shape[1:] or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor of src's dtype and trailing shape")
        with torch.no_grad():
            x = _rows(src)
            _gather(x, None, indptr, out.shape[0], out=out.view(out.shape[0], x.shape[1]))
        return out
    N = int(indptr[-1])
    return _Gather.apply(src, None, indptr, N)


# ---- torch_scatter: index route -------------------------------------------------------------------------------------------

def _check_index(src, index, dim):
    if not isinstance(src, torch.Tensor) or not isinstance(index, torch.Tensor):
        raise TypeError("src and index must be tensors")
    if dim not in (0, -src.dim()):
        raise NotImplementedError(f"only dim=0 is supported, not dim={dim}")
    _check_src(src)
    if not index.is_cuda or index.device != src.device:
        raise RuntimeError(_NO_CPU if not index.is_cuda else "index must live on src's device")
    if index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool:
        raise TypeError(f"index must be an integer tensor, not {index.dtype}")
    if index.dim() != 1:       # a broadcast of a 1-D index along dim 0: every other dimension has size 1 or stride 0
        if index.dim() != src.dim() or any(n != 1 and s != 0 for n, s in zip(index.shape[1:], index.stride()[1:])):
            raise NotImplementedError("index must be 1-D, or a 1-D index broadcast along dim 0")
        index = index[(slice(None),) + (0,) * (index.dim() - 1)]
    if index.shape[0] != src.shape[0]:
        raise ValueError(f"index has {index.shape[0]} entries for {src.shape[0]} rows of src")
    return index.long().contiguous()


def _dim_size(index, out, dim_size):
    if out is not None:
        return out.shape[0]
    if dim_size is not None:
        return int(dim_size)
    return int(index.max()) + 1 if index.numel() else 0


def _scatter(src, index, dim, out, dim_size, op):
    index = _check_index(src, index, dim)
    S = _dim_size(index, out, dim_size)
    perm, indptr = _sorted_route(index, S)
    res, arg = _Reduce.apply(src, perm, indptr, op)
    if out is not None:
        # upstream reduces into what `out` holds; here `out` is a destination only
        out.copy_(res)
        res = out
    return res, arg


def scatter_sum(src, index, dim=0, out=None, dim_size=None):
    return _scatter(src, index, dim, out, dim_size, "sum")[0]


scatter_add = scatter_sum


def scatter_mean(src, index, dim=0, out=None, dim_size=None):
    return _scatter(src, index, dim, out, dim_size, "mean")[0]


def scatter_min(src, index, dim=0, out=None, dim_size=None):
    return _scatter(src, index, dim, out, dim_size, "min")


def scatter_max(src, index, dim=0, out=None, dim_size=None):
    return _scatter(src, index, dim, out, dim_size, "max")


def scatter_std(src, index, dim=0, out=None, dim_size=None, unbiased=True):
    """Two passes over the primitives: the per-segment mean, then sqrt(sum of squared deviations / (count' + 1e-6)) with
    count' = clamp(count - 1, 1) if unbiased else count."""
    index = _check_index(src, index, dim)
    if src.dtype == torch.int64:
        raise TypeError("scatter_std needs a floating dtype")
    S = _dim_size(index, out, dim_size)
    perm, indptr = _sorted_route(index, S)
    mean, _ = _Reduce.apply(src, perm, indptr, "mean")
    dev = src - _Gather.apply(mean, perm, indptr, src.shape[0])
    sum_sq, _ = _Reduce.apply(dev * dev, perm, indptr, "sum")
    count = (indptr[1:] - indptr[:-1]).float()         # fp32 whatever src is: fp16 / bf16 cannot hold the counts
    count = (count - 1).clamp_(min=1) if unbiased else count
    res = torch.sqrt(sum_sq.float() / (count.view((S,) + (1,) * (src.dim() - 1)) + 1e-6)).to(src.dtype)
    return _finish(res, out)


def scatter(src, index, dim=0, out=None, dim_size=None, reduce="sum"):
    """torch_scatter.scatter: reduce the rows of src that share an index; min / max return the values only."""
    if reduce == "add":
        reduce = "sum"
    if reduce not in L.GDR_SEG_OPS:
        raise ValueError(f"reduce must be one of sum, add, mean, min, max; got {reduce!r}")
    return _scatter(src, index, dim, out, dim_size, reduce)[0]


# ---- torch_geometric.utils ------------------------------------------------------------------------------------------------

def pyg_scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    """torch_geometric.utils.scatter (no `out`)."""
    return scatter(src, index, dim=dim, dim_size=dim_size, reduce=reduce)


def softmax(src, index=None, ptr=None, num_nodes=None, dim=0):
    """torch_geometric.utils.softmax: the softmax of src over the rows of each group, given by `ptr` (CSR) or by `index`."""
    if isinstance(src, torch.Tensor) and dim not in (0, -src.dim()):
        raise NotImplementedError(f"only dim=0 is supported, not dim={dim}")
    if ptr is not None:
        _check_ptr_layout(ptr)
    _check_src(src)
    if src.dtype == torch.int64:
        raise TypeError("softmax needs a floating dtype")
    if ptr is not None:
        return _Softmax.apply(src, None, _check_ptr(ptr, src))
    if index is None:
        raise ValueError("softmax needs `index` or `ptr`")
    index = _check_index(src, index, dim)
    S = int(num_nodes) if num_nodes is not None else (int(index.max()) + 1 if index.numel() else 0)
    perm, indptr = _sorted_route(index, S)
    return _Softmax.apply(src, perm, indptr)


def cumsum(x, dim=0):
    """torch_geometric.utils.cumsum: the cumulative sum along `dim` behind a leading zero (one entry longer than x)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a tensor, not {type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError(_NO_CPU)
    size = list(x.shape)
    size[dim] += 1
    out = x.new_zeros(size)
    torch.cumsum(x, dim=dim, out=out.narrow(dim, 1, x.shape[dim]))
    return out
