"""GPU: the fused glue of UpscaleModule (csrc/upscale.hip through generativedensification_amd.upscale) against the float64
restatement (tests/upscale_ref.py) and against the torch composition on the same GPU in the same dtypes.

Accuracy bar, for every output and gradient: with e_hip = max|hip - ref64| and e_torch = max|torch - ref64| (ref64 on the inputs
as rounded to their dtypes), e_hip <= 2 e_torch + half an ulp of the result dtype at max|ref64|.  The maxima are pooled over
the draws of a case (tests/upscale_cases.py: every judged tensor has at least 256 elements in all); every pooled pair is printed
before it is asserted.  Directly under the bar: out_x, grad_t, grad_coord and all of merge.

What sits behind the PE argument is judged differently: sin(2^14 x) turns a last-bit difference in x into 1e-5 (fp32) up to 0.3
(bf16) of the result, so against a truth at the unrounded x the bar would pass anything.  h and grad_feat of `expand` must equal
BITWISE what norm.pe_concat_layer_norm returns for the PE argument the call itself produced (out_x; taken with coord = 0 for the
relative PE, where 0 + d is exact) and the same grad_h; grad_t and grad_coord are judged against the float64 chain rule applied
to that call's dx (the torch composition against the chain rule applied to its own gradient at delta_x)."""
import copy
import types

import numpy as np
import pytest
import torch

import upscale_cases as UC
import upscale_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GRID = UC.GRID_SIZE

# dtype sets: name -> (dtypes of t / skip / branch / scale / keep, of feat / coord / frequencies, autocast).  The trainer's set
# runs under bf16 autocast, where the results and so the upstream gradients are float32.
SETS = {"f32": (F32, F32, False), "f16": (F16, F16, False), "trainer": (BF16, F32, True)}


def upscale():
    from generativedensification_amd import upscale as U

    return U


def norm():
    from generativedensification_amd import norm as N

    return N


def dev(a, dtype=None):
    return R.to_dtype(a, dtype).to(DEV) if dtype is not None else torch.as_tensor(np.asarray(a)).to(DEV)


def f64(t):
    return t.detach().double().cpu().numpy()


def leaf(t):
    return t.clone().requires_grad_(True)


class Pool:
    """the maxima of a case over its draws, per judged tensor"""

    def __init__(self):
        self.rows = {}

    def add(self, what, hip, ref_hip, tor, ref_tor=None):
        ref_tor = ref_hip if ref_tor is None else ref_tor
        assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref_hip.shape == ref_tor.shape, (what, hip.dtype, tor.dtype, hip.shape,
                                                                                                 tor.shape, ref_hip.shape)
        assert np.isfinite(f64(hip)).all(), what
        row = self.rows.setdefault(what, [0.0, 0.0, 0.0, hip.dtype, 0])
        if ref_hip.size:
            row[0] = max(row[0], float(np.abs(f64(hip) - ref_hip).max()))
            row[1] = max(row[1], float(np.abs(f64(tor) - ref_tor).max()))
            row[2] = max(row[2], float(np.abs(ref_hip).max()))
        row[4] += ref_hip.size

    def settle(self, tag):
        bad = []
        for what, (e_hip, e_torch, mag, dtype, count) in self.rows.items():
            slack = R.half_ulp(dtype, mag)
            print(f"upscale-bar {tag}/{what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e} elements={count}")
            assert count >= 256, (what, count)
            if not e_hip <= 2 * e_torch + slack:
                bad.append((what, e_hip, e_torch, slack))
        assert not bad, bad


# ---- expand ---------------------------------------------------------------------------------------------------------------

def expand_once(name, set_name, draw, pool):
    U, N = upscale(), norm()
    lo, hi, autocast = SETS[set_name]
    t64, coord64, feat64, freq64, s, absolute, gx64, gh64 = UC.expand_inputs(name, draw)
    t, coord, feat, freq = dev(t64, lo), dev(coord64, hi), dev(feat64, hi), dev(freq64, hi)
    if lo == F16:
        # the gradient at x carries the factor 2^(F - 1): with a unit grad_h its sum over the children of a parent (grad_coord
        # under absolute_pe) passes float16's largest number, 65504, in the truth itself
        gh64 = gh64 * 2.0 ** -6
    ins = [leaf(a) for a in (t, coord, feat)]
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        out_x, h = U.expand(*ins, freq, s, GRID, absolute)
    kept = {}
    t_ins = [leaf(a) for a in (t, coord, feat)]
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        t_out_x, t_h = R.torch_expand(*t_ins, freq, s, GRID, absolute, keep=kept)
    assert out_x.dtype == t_out_x.dtype and h.dtype == t_h.dtype and h.shape == t_h.shape, (out_x.dtype, t_out_x.dtype, h.dtype, t_h.dtype)
    assert h.stride(1) == 1 and h.stride(0) % 8 == 0 and out_x.is_contiguous()
    gx, gh = dev(gx64, out_x.dtype), dev(gh64, h.dtype)
    torch.autograd.backward([out_x, h], [gx, gh])
    torch.autograd.backward([t_out_x, t_h], [gx, gh])
    for a, b in zip(ins, (t, coord, feat)):
        assert a.grad.dtype == b.dtype and a.grad.shape == b.shape
    r_t, r_coord = f64(t), f64(coord)
    pool.add("out_x", out_x, R.expand(r_t, r_coord, f64(feat), f64(freq), s, GRID, absolute)[0], t_out_x)
    # the PE argument the call itself produced, and pe_concat_layer_norm at it: the same bits
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16, enabled=autocast):
        x_arg = out_x.detach().clone() if absolute else U.expand(t, torch.zeros_like(coord, dtype=lo), feat, freq, s, GRID, False)[0]
    x_arg.requires_grad_(True)
    p_feat = leaf(feat)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        pe = N.pe_concat_layer_norm(x_arg, p_feat, freq, s)
    assert pe.dtype == h.dtype and pe.stride() == h.stride()
    assert torch.equal(pe, h), f"h differs from pe_concat_layer_norm at the call's own argument: {float((pe - h).abs().max())}"
    pe.backward(gh)
    assert torch.equal(p_feat.grad, ins[2].grad), "grad_feat differs from pe_concat_layer_norm's"
    # grad_t, grad_coord: the float64 chain rule at each candidate's own gradient behind the PE
    g64 = f64(gx)
    ref_t, ref_coord = R.expand_chain(r_t, GRID, s, g64, f64(x_arg.grad), absolute)
    zero = np.zeros_like(g64)
    tor_t = R.expand_chain(r_t, GRID, s, zero, f64(kept["delta_x"].grad), True)[0]
    tor_coord = f64(kept["skip_x"].grad).reshape(-1, s, 3).sum(1)
    pool.add("grad_t", ins[0].grad, ref_t, t_ins[0].grad, tor_t)
    pool.add("grad_coord", ins[1].grad, ref_coord, t_ins[1].grad, tor_coord)
    return (out_x, h, ins[0].grad, ins[1].grad, ins[2].grad)


def run_expand(name, set_name):
    pool = Pool()
    for draw in range(UC.expand_draws(name)):
        expand_once(name, set_name, draw, pool)
    pool.settle(f"expand/{name}/{set_name}")


@pytest.mark.parametrize("name", list(UC.EXPAND))
def test_expand_f32_at_every_shape(name):
    run_expand(name, "f32")


@pytest.mark.parametrize("set_name", ["f16", "trainer"])
@pytest.mark.parametrize("name", UC.EXPAND_DTYPE_CASES)
def test_expand_16_bit(name, set_name):
    run_expand(name, set_name)


# ---- merge ----------------------------------------------------------------------------------------------------------------

def merge_once(name, set_name, draw, pool):
    U = upscale()
    lo, _, autocast = SETS[set_name]
    skip64, branch64, keep64, scale64, offset, s, g64 = UC.merge_inputs(name, draw)
    skip, branch, scale = dev(skip64, lo), dev(branch64, lo), dev(scale64, lo)
    keep = None if keep64 is None else (dev(keep64, lo) if draw % 2 == 0 else dev(keep64, lo).reshape(-1, 1))      # (N S,) and (N S, 1)
    off = dev(offset)
    ins = [leaf(a) for a in (skip, branch, scale)]
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        out = U.merge(ins[0], ins[1], keep, ins[2], off, s)
    t_ins = [leaf(a) for a in (skip, branch, scale)]
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        t_out = R.torch_merge(t_ins[0], t_ins[1], keep, t_ins[2], off, s)
    assert out.dtype == t_out.dtype and out.is_contiguous()
    g = dev(g64, out.dtype)
    out.backward(g)
    t_out.backward(g)
    r = (f64(skip), f64(branch), None if keep is None else f64(keep).reshape(-1), f64(scale))
    pool.add("out", out, R.merge(*r, offset, s), t_out)
    for what, a, b, ref in zip(("grad_skip", "grad_branch", "grad_scale"), ins, t_ins, R.merge_grad(*r, offset, s, f64(g))):
        assert a.grad.dtype == lo
        pool.add(what, a.grad, ref, b.grad)
    n = skip.shape[0]
    seg = np.searchsorted(offset, np.arange(n), side="right")
    tail = torch.as_tensor(seg >= len(offset)).to(DEV)
    assert not out[tail.repeat_interleave(s)].any() and not ins[1].grad[tail.repeat_interleave(s)].any() and not ins[0].grad[tail].any()
    empty = torch.as_tensor(np.bincount(seg, minlength=len(offset) + 1)[:len(offset)] == 0).to(DEV)
    assert not ins[2].grad[empty].any(), "empty segments"
    return (out, ins[0].grad, ins[1].grad, ins[2].grad)


def run_merge(name, set_name):
    pool = Pool()
    for draw in range(UC.merge_draws(name)):
        merge_once(name, set_name, draw, pool)
    pool.settle(f"merge/{name}/{set_name}")


@pytest.mark.parametrize("name", list(UC.MERGE))
def test_merge_f32_at_every_shape(name):
    run_merge(name, "f32")


@pytest.mark.parametrize("set_name", ["f16", "trainer"])
@pytest.mark.parametrize("name", UC.MERGE_DTYPE_CASES)
def test_merge_16_bit(name, set_name):
    run_merge(name, set_name)


def test_merge_mixed_dtypes_round_as_the_composition():
    """skip float32 with a bf16 branch: y is float32 (the promotion) and grad_branch comes back bf16"""
    U = upscale()
    pool = Pool()
    skip64, branch64, keep64, scale64, offset, s, g64 = UC.merge_inputs("c256_s4_b3")
    skip, branch, keep, scale, off = dev(skip64, F32), dev(branch64, BF16), dev(keep64, BF16), dev(scale64, F32), dev(offset)
    ins, t_ins = [leaf(a) for a in (skip, branch, scale)], [leaf(a) for a in (skip, branch, scale)]
    out, t_out = U.merge(ins[0], ins[1], keep, ins[2], off, s), R.torch_merge(t_ins[0], t_ins[1], keep, t_ins[2], off, s)
    assert out.dtype == t_out.dtype == F32
    g = dev(g64, F32)
    out.backward(g)
    t_out.backward(g)
    r = (f64(skip), f64(branch), f64(keep), f64(scale))
    pool.add("out", out, R.merge(*r, offset, s), t_out)
    for what, a, b, ref in zip(("grad_skip", "grad_branch", "grad_scale"), ins, t_ins, R.merge_grad(*r, offset, s, f64(g))):
        assert a.grad.dtype == b.grad.dtype
        pool.add(what, a.grad, ref, b.grad)
    pool.settle("merge/c256_s4_b3/mixed")


@pytest.mark.parametrize("dtypes", [(F32, F32), (BF16, F32), (F16, F16)], ids=str)
@pytest.mark.parametrize("shape", [(300, 160, [120, 257]), (70, 776, [17, 17, 70]), (5000, 8, [4999, 5000])], ids=str)
def test_degenerate_merge_is_ada_layer_norm_bitwise(shape, dtypes):
    """upscale_factor = 1, keep = None and a zero skip: the LayerNorm passes are the shared ones, so forward and every gradient
    equal ada_layer_norm's bit for bit"""
    U, N = upscale(), norm()
    n, c, offset = shape
    rng = np.random.default_rng(n + c)
    feat, scale = dev(rng.standard_normal((n, c)) * 1.5 + 0.25, dtypes[0]), dev(rng.standard_normal((len(offset), c)), dtypes[1])
    off = dev(np.asarray(offset, dtype=np.int64))
    a, b = leaf(feat), leaf(scale)
    want = N.ada_layer_norm(a, b, off)
    g = dev(rng.standard_normal((n, c)), want.dtype)
    want.backward(g)
    x, y = leaf(feat), leaf(scale)
    got = U.merge(torch.zeros_like(feat), x, None, y, off, 1)
    got.backward(g)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(x.grad, a.grad) and torch.equal(y.grad, b.grad)


# ---- properties -----------------------------------------------------------------------------------------------------------

def test_two_calls_are_bitwise_equal():
    runs = [expand_once("c256_s4_abs", "trainer", 0, Pool()) + merge_once("c256_s4_b3", "trainer", 1, Pool()) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_a_one_parent_call_equals_the_first_rows_of_a_larger_call():
    U = upscale()
    rng = np.random.default_rng(17)
    n, s, c, f = 17, 3, 40, 15
    t, coord, feat = dev(rng.standard_normal((n, 3 * s)), BF16), dev(rng.uniform(-0.5, 0.5, (n, 3)), F32), dev(rng.standard_normal((n, c)), F32)
    freq = dev(2.0 ** np.arange(f), F32)
    for absolute in (False, True):
        big, one = U.expand(t, coord, feat, freq, s, GRID, absolute), U.expand(t[:1], coord[:1], feat[:1], freq, s, GRID, absolute)
        assert torch.equal(one[0], big[0][:s]) and torch.equal(one[1], big[1][:s])
    skip, branch, scale = dev(rng.standard_normal((n, c)), BF16), dev(rng.standard_normal((n * s, c)), BF16), dev(rng.standard_normal((1, c)), F32)
    keep = dev((rng.uniform(size=n * s) < 0.7) / 0.7, BF16)
    big = U.merge(skip, branch, keep, scale, dev(np.array([n])), s)
    one = U.merge(skip[:1], branch[:s], keep[:s], scale, dev(np.array([1])), s)
    assert torch.equal(one, big[:s])


def guarded(rows, cols, dtype, fill=7.0, guard=16):
    full = torch.full((rows + 2 * guard, cols), fill, dtype=dtype, device=DEV)
    return full, full[guard:guard + rows]


def guards_kept(full, rows, fill=7.0, guard=16):
    return bool((full[:guard] == fill).all()) and bool((full[guard + rows:] == fill).all())


def test_guard_rows_round_every_output_keep_their_fill():
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M

    lib = L.load()
    dt = {F32: L.GDR_NORM_DTYPES["f32"], BF16: L.GDR_NORM_DTYPES["bf16"]}
    rng = np.random.default_rng(5)
    n, s, c, f = 33, 3, 40, 15
    w, wp = 6 * f + c, (6 * f + c + 7) // 8 * 8
    t, coord, feat = dev(rng.standard_normal((n, 3 * s)), BF16), dev(rng.uniform(-0.5, 0.5, (n, 3)), F32), dev(rng.standard_normal((n, c)), F32)
    freq = dev(2.0 ** np.arange(f), F32)
    ox_full, ox = guarded(n * s, 3, F32)
    h_full, h = guarded(n * s, wp, F32)
    L.check(lib.gdr_upscale_expand_forward(t.data_ptr(), dt[BF16], coord.data_ptr(), dt[F32], feat.data_ptr(), c, dt[F32], freq.data_ptr(),
                                           dt[F32], n, s, c, f, 0.5 * GRID, 1, 1e-5, ox.data_ptr(), dt[F32], h.data_ptr(), wp, dt[F32],
                                           M.stream()), "expand_forward")
    gt_full, gt = guarded(n, 3 * s, BF16)
    gc_full, gc = guarded(n, 3, F32)
    gf_full, gf = guarded(n, c, F32)
    gh, gx = dev(rng.standard_normal((n * s, wp)), F32), dev(rng.standard_normal((n * s, 3)), F32)
    L.check(lib.gdr_upscale_expand_backward(gh.data_ptr(), wp, dt[F32], gx.data_ptr(), dt[F32], t.data_ptr(), dt[BF16], coord.data_ptr(),
                                            dt[F32], feat.data_ptr(), c, dt[F32], freq.data_ptr(), dt[F32], n, s, c, f, 0.5 * GRID, 1, 1e-5,
                                            gt.data_ptr(), gc.data_ptr(), gf.data_ptr(), M.stream()), "expand_backward")
    torch.cuda.synchronize()
    assert guards_kept(ox_full, n * s) and guards_kept(h_full, n * s) and guards_kept(gt_full, n) and guards_kept(gc_full, n) and guards_kept(gf_full, n)
    assert not (ox == 7.0).any() and not (h[:, :w] == 7.0).any() and not h[:, w:].any() and not (gf == 7.0).any() and not (gc == 7.0).any()
    want = upscale().expand(t, coord, feat, freq, s, GRID, True)
    assert torch.equal(ox, want[0]) and torch.equal(h[:, :w], want[1])
    # merge, with parents behind the last end (their rows are written as zeros, not left)
    skip, branch = dev(rng.standard_normal((n, c)), BF16), dev(rng.standard_normal((n * s, c)), BF16)
    keep, scale = dev((rng.uniform(size=n * s) < 0.7) / 0.7, BF16), dev(rng.standard_normal((3, c)), F32)
    off = dev(np.array([10, 10, 30]))
    out_full, out = guarded(n * s, c, F32)
    L.check(lib.gdr_upscale_merge_forward(skip.data_ptr(), c, dt[BF16], branch.data_ptr(), c, dt[BF16], keep.data_ptr(), dt[BF16],
                                          scale.data_ptr(), c, dt[F32], off.data_ptr(), n, s, 3, c, 1e-5, out.data_ptr(), dt[F32],
                                          M.stream()), "merge_forward")
    gs_full, gs = guarded(n, c, BF16)
    gb_full, gb = guarded(n * s, c, BF16)
    gsc_full, gsc = guarded(3, c, F32)
    g = dev(rng.standard_normal((n * s, c)), F32)
    nbytes = lib.gdr_upscale_merge_backward_bytes(n, s, 3, c)
    assert nbytes > 0
    ws, base, usable = M.workspace(nbytes, DEV)
    L.check(lib.gdr_upscale_merge_backward(g.data_ptr(), c, dt[F32], skip.data_ptr(), c, dt[BF16], branch.data_ptr(), c, dt[BF16],
                                           keep.data_ptr(), dt[BF16], scale.data_ptr(), c, dt[F32], off.data_ptr(), n, s, 3, c, 1e-5, base,
                                           usable, gs.data_ptr(), gb.data_ptr(), gsc.data_ptr(), M.stream()), "merge_backward")
    torch.cuda.synchronize()
    assert guards_kept(out_full, n * s) and guards_kept(gs_full, n) and guards_kept(gb_full, n * s) and guards_kept(gsc_full, 3)
    assert not (out == 7.0).any() and not (gs == 7.0).any() and not (gb == 7.0).any() and not (gsc == 7.0).any()
    assert not out[30 * s:].any() and not gs[30:].any() and not gb[30 * s:].any() and not gsc[1].any()


def test_unneeded_gradients_are_not_stored_and_none_gradients_read_as_zeros(monkeypatch):
    U = upscale()
    from generativedensification_amd import _lib as L

    lib = L.load()
    seen = []

    def spy_on(name):
        real = getattr(lib, name)

        def spy(*args):
            seen.append(args)
            return real(*args)

        monkeypatch.setattr(lib, name, spy)

    t64, coord64, feat64, freq64, s, absolute, gx64, gh64 = UC.expand_inputs("c160_s2")
    t, coord, feat, freq = dev(t64, F32), dev(coord64, F32), dev(feat64, F32), dev(freq64, F32)
    gx, gh = dev(gx64, F32), dev(gh64, F32)
    full = [leaf(a) for a in (t, coord, feat)]
    torch.autograd.backward(list(U.expand(*full, freq, s, GRID, absolute)), [gx, gh])
    spy_on("gdr_upscale_expand_backward")
    a = leaf(t)
    torch.autograd.backward(list(U.expand(a, coord, feat, freq, s, GRID, absolute)), [gx, gh])
    grad_t, grad_coord, grad_feat = seen[-1][-4:-1]
    assert grad_t is not None and grad_coord is None and grad_feat is None and torch.equal(a.grad, full[0].grad)
    b = leaf(feat)
    torch.autograd.backward(list(U.expand(t, coord, b, freq, s, GRID, absolute)), [gx, gh])
    assert seen[-1][-4] is None and seen[-1][-3] is None and seen[-1][-2] is not None and torch.equal(b.grad, full[2].grad)
    # only out_x is used: grad_h reaches the kernel as NULL and reads as zeros; grad_feat is exactly zero, grad_coord the child sum
    only = [leaf(v) for v in (t, coord, feat)]
    U.expand(*only, freq, s, GRID, False)[0].backward(gx)
    assert seen[-1][0] is None and seen[-1][3] is not None
    assert not only[2].grad.any() and torch.allclose(only[1].grad, gx.reshape(-1, s, 3).sum(1))
    ref_t = R.expand_grad(f64(t), f64(coord), f64(feat), f64(freq), s, GRID, f64(gx), None, False)[0]
    assert np.abs(f64(only[0].grad) - ref_t).max() <= 1e-6 * np.abs(ref_t).max()
    # only h is used: grad_out_x is NULL
    only = [leaf(v) for v in (t, coord, feat)]
    U.expand(*only, freq, s, GRID, False)[1].backward(gh)
    assert seen[-1][0] is not None and seen[-1][3] is None and not only[1].grad.any()
    # merge
    skip64, branch64, keep64, scale64, offset, s, g64 = UC.merge_inputs("c8_s3_b3")
    skip, branch, keep, scale, off, g = dev(skip64, F32), dev(branch64, F32), dev(keep64, F32), dev(scale64, F32), dev(offset), dev(g64, F32)
    full = [leaf(v) for v in (skip, branch, scale)]
    U.merge(full[0], full[1], keep, full[2], off, s).backward(g)
    spy_on("gdr_upscale_merge_backward")
    for i in range(3):
        ins = [skip, branch, scale]
        ins[i] = leaf(ins[i])
        U.merge(ins[0], ins[1], keep, ins[2], off, s).backward(g)
        outs = seen[-1][-4:-1]
        assert [o is not None for o in outs] == [j == i for j in range(3)]
        assert torch.equal(ins[i].grad, full[i].grad)


def test_no_host_synchronisation():
    U, N = upscale(), norm()
    m = R.make_module(160, 256, 2, 15, drop_path=0.3, residual_attribute=True, is_first=False, ada_forward=N.ada_layer_norm_forward).to(DEV)
    m.train()
    coord64, feat64, glob64, offset = UC.module_inputs(65, 160, 3)
    coord, glob, off = dev(coord64, F32), dev(glob64, F32), dev(offset)
    attribute = torch.zeros(65, 11, device=DEV)

    def call(feat):
        point = R.Point(coord=coord, feat=feat, global_feat=glob, offset=off, grid_size=GRID, attribute=attribute)
        with torch.autocast("cuda", dtype=BF16):
            out = U.upscale_res_module_forward(m, point)
        (out.feat.float().sum() + out.coord.sum()).backward()
        return out

    old = U.UPSCALE_BACKEND
    U.UPSCALE_BACKEND = "hip"
    try:
        call(dev(feat64, F32).requires_grad_(True))          # warm-up: library load, kernel images, the GEMMs
        feat = dev(feat64, F32).requires_grad_(True)
        m.zero_grad()
        torch.cuda.synchronize()
        previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            raised = False
            try:
                off[-1].item()                               # the canary: what gather_csr's read-back does
            except RuntimeError:
                raised = True
            if raised:
                out = call(feat)
        finally:
            torch.cuda.set_sync_debug_mode(previous)
    finally:
        U.UPSCALE_BACKEND = old
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
    torch.cuda.synchronize()
    assert out.feat.shape == (130, 256) and out.attribute.shape == (130, 11) and torch.equal(out.offset, off * 2)
    assert torch.isfinite(feat.grad).all() and torch.isfinite(m.skip.weight.grad).all()


def test_runs_under_vjp_and_under_no_grad_and_autocast_gives_the_documented_dtypes():
    U = upscale()
    t64, coord64, feat64, freq64, s, absolute, gx64, gh64 = UC.expand_inputs("c40_s3_abs")
    t, coord, feat, freq, gx, gh = (dev(a, F32) for a in (t64, coord64, feat64, freq64, gx64, gh64))
    fn = lambda a, b, c: U.expand(a, b, c, freq, s, GRID, absolute)      # noqa: E731
    outs, grads = torch.autograd.functional.vjp(fn, (t, coord, feat), (gx, gh))
    ins = [leaf(a) for a in (t, coord, feat)]
    o = fn(*ins)
    torch.autograd.backward(list(o), [gx, gh])
    assert all(torch.equal(a, b) for a, b in zip(outs, o)) and all(torch.equal(a, b.grad) for a, b in zip(grads, ins))
    with torch.no_grad():
        again = fn(*ins)
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(again, o))
    skip64, branch64, keep64, scale64, offset, ms, g64 = UC.merge_inputs("c8_s3_b3")
    skip, branch, keep, scale, g = (dev(a, F32) for a in (skip64, branch64, keep64, scale64, g64))
    off = dev(offset)
    mfn = lambda a, b, c: U.merge(a, b, keep, c, off, ms)      # noqa: E731
    out, grads = torch.autograd.functional.vjp(mfn, (skip, branch, scale), g)
    ins = [leaf(a) for a in (skip, branch, scale)]
    o = mfn(*ins)
    o.backward(g)
    assert torch.equal(out, o) and all(torch.equal(a, b.grad) for a, b in zip(grads, ins))
    with torch.no_grad():
        assert torch.equal(mfn(*ins), o) and not mfn(*ins).requires_grad
    # dtypes: the compositions', with and without autocast
    for autocast in (False, True):
        for lo, hi in ((F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, BF16)):
            with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                got = U.expand(t.to(lo), coord.to(hi), feat.to(hi), freq, s, GRID, absolute)
                want = R.torch_expand(t.to(lo), coord.to(hi), feat.to(hi), freq, s, GRID, absolute)
                mgot = U.merge(skip.to(hi), branch.to(lo), keep.to(lo), scale.to(lo), off, ms)
                mwant = R.torch_merge(skip.to(hi), branch.to(lo), keep.to(lo), scale.to(lo), off, ms)
            assert got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype and mgot.dtype == mwant.dtype, (autocast, lo, hi)
            if autocast:
                assert got[1].dtype == F32 and mgot.dtype == F32


def test_refusals_come_before_the_library_is_loaded_and_empty_inputs_return_empty_tensors(monkeypatch):
    U = upscale()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    z = lambda *shape, dtype=F32: torch.zeros(*shape, dtype=dtype, device=DEV)      # noqa: E731
    freq = torch.ones(3, device=DEV)
    good = (z(4, 6), z(4, 3), z(4, 16), freq, 2, GRID)
    for i in (0, 1, 2, 3):
        bad = list(good)
        bad[i] = bad[i].double()
        with pytest.raises(TypeError):
            U.expand(*bad)
    for bad in ((z(4, 9),) + good[1:], good[:2] + (z(4, 12),) + good[3:], good[:2] + (z(4, 1032),) + good[3:], good[:3] + (torch.ones(17, device=DEV),) + good[4:],
                (z(4, 51),) + good[1:4] + (17, GRID), good[:1] + (z(5, 3),) + good[2:]):
        with pytest.raises(ValueError):
            U.expand(*bad)
    with pytest.raises(NotImplementedError):
        U.expand(*good[:3], torch.ones(0, device=DEV), 2, GRID)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.expand(good[0].cpu(), *good[1:])
    mgood = (z(4, 16), z(8, 16), None, z(1, 16), torch.tensor([4], device=DEV), 2)
    with pytest.raises(TypeError):
        U.merge(mgood[0].double(), *mgood[1:])
    with pytest.raises(TypeError):
        U.merge(*mgood[:4], torch.tensor([4.0], device=DEV), 2)
    for bad in (mgood[:1] + (z(9, 16),) + mgood[2:], mgood[:3] + (z(2, 16),) + mgood[4:], mgood[:2] + (z(5),) + mgood[3:],
                (z(4, 12), z(8, 12), None, z(1, 12)) + mgood[4:], mgood[:5] + (17,)):
        with pytest.raises(ValueError):
            U.merge(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.merge(*mgood[:4], torch.tensor([4]), 2)
    # empties: no library, no launch
    out_x, h = U.expand(z(0, 6), z(0, 3), z(0, 16, dtype=BF16), freq, 2, GRID)
    assert out_x.shape == (0, 3) and h.shape == (0, 34) and h.dtype == F32
    out = U.merge(z(0, 16), z(0, 16, dtype=BF16), None, z(2, 16), torch.tensor([0, 0], device=DEV), 2)
    assert out.shape == (0, 16) and out.dtype == F32


# ---- the bound forwards ---------------------------------------------------------------------------------------------------

def module_and_point(c, co, s, f, n, b, dtype=F32, grad=False, **kw):
    N = norm()
    m = R.make_module(c, co, s, f, ada_forward=N.ada_layer_norm_forward, **kw).to(DEV)
    coord64, feat64, glob64, offset = UC.module_inputs(n, c, b)

    def point(module_dtype=dtype, device=DEV):
        feat = R.to_dtype(feat64, module_dtype).to(device).requires_grad_(grad)
        coord = R.to_dtype(coord64, module_dtype).to(device).requires_grad_(grad)
        p = R.Point(coord=coord, feat=feat, global_feat=R.to_dtype(glob64, module_dtype).to(device),
                    offset=torch.as_tensor(offset).to(device), grid_size=GRID)
        if kw.get("residual_attribute"):
            p["attribute"] = torch.arange(n * 5, dtype=module_dtype, device=device).reshape(n, 5)
        return p

    return m, point


def with_backend(name, fn):
    U = upscale()
    old = U.UPSCALE_BACKEND
    U.UPSCALE_BACKEND = name
    try:
        return fn()
    finally:
        U.UPSCALE_BACKEND = old


@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16_autocast"])
def test_bound_forward_under_hip_is_the_composition_of_the_public_pieces(autocast):
    U = upscale()
    m, point = module_and_point(160, 256, 2, 15, 65, 3, drop_path=0.25, absolute_pe=True, residual_attribute=True, is_first=False)
    m.train()
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        torch.manual_seed(11)
        got = with_backend("hip", lambda: U.upscale_res_module_forward(m, point()))
        torch.manual_seed(11)
        p = m.in_norm(point())
        out_x, h = U.expand(m.delta_x(p.feat), p.coord, p.feat, m.frequencies, 2, GRID, True, m.delta_f[0].eps)
        branch = m.delta_f[1:](h)
        keep = branch.new_empty((branch.shape[0], 1)).bernoulli_(0.75).div_(0.75)
        feat = U.merge(m.skip(p.feat), branch, keep, m.out_norm[0].affine(p.global_feat), p.offset, 2, m.out_norm[0].eps)
    assert torch.equal(got.coord, out_x) and torch.equal(got.feat, feat) and torch.equal(got.offset, p.offset * 2)
    assert torch.equal(got.attribute, point().attribute.repeat_interleave(2, 0))
    assert got.feat.dtype == F32 and got.coord.dtype == F32 and not (keep == 0).all() and (keep == 0).any()


@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16_autocast"])
def test_bound_forward_under_torch_is_the_reference_restated_and_the_generator_ends_in_the_same_state(autocast):
    U = upscale()
    import torch_scatter

    m, point = module_and_point(40, 8, 3, 15, 33, 3, drop_path=0.25, residual_attribute=True, is_first=False)
    m.train()
    states = {}
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        torch.manual_seed(5)
        want = R.reference_forward(m, point(), res=True, gather=torch_scatter.gather_csr)
        states["reference"] = torch.cuda.get_rng_state(DEV)
        for backend in ("torch", "hip"):
            torch.manual_seed(5)
            got = with_backend(backend, lambda: U.upscale_res_module_forward(m, point()))
            states[backend] = torch.cuda.get_rng_state(DEV)
            if backend == "torch":
                assert all(torch.equal(got[k], want[k]) for k in ("coord", "feat", "offset", "attribute"))
            else:
                assert got.feat.shape == want.feat.shape and torch.isfinite(got.feat).all() and torch.equal(got.attribute, want.attribute)
    assert torch.equal(states["torch"], states["reference"]) and torch.equal(states["hip"], states["reference"])
    # outside covers() the hip backend runs the reference's lines: the same bits
    m.delta_f[2] = torch.nn.ReLU()
    assert not U.covers(m)
    m.eval()
    want = R.reference_forward(m, point(), res=True, gather=torch_scatter.gather_csr)
    got = with_backend("hip", lambda: U.upscale_res_module_forward(m, point()))
    assert torch.equal(got.feat, want.feat) and torch.equal(got.coord, want.coord)


@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16_autocast"])
def test_both_backends_meet_the_bar_against_a_float64_copy_of_the_module(autocast):
    """F = 2: the PE amplifies a last-bit difference of x by 4 at most, so the whole module is under the bar"""
    U = upscale()
    pool = Pool()
    for seed in range(3):
        m, point = module_and_point(40, 8, 3, 2, 33, 3, grad=True, seed=seed)
        m.eval()
        m64 = copy.deepcopy(m).double().cpu()
        for mod in (m64.in_norm[0], m64.out_norm[0]):
            mod.forward = types.MethodType(lambda self, feat, g, offset: R.torch_ada(feat, self.affine(g), offset, self.eps), mod)
        watched = lambda mod: [mod.skip.weight, mod.delta_x[2].weight, mod.delta_f[1].weight, mod.out_norm[0].affine.weight]      # noqa: E731
        p64 = point(torch.float64, "cpu")
        leaves64 = [p64.feat, p64.coord]                     # (kept here: the forward rebinds point.feat / point.coord)
        ref = R.reference_forward(m64, p64)
        rng = np.random.default_rng(seed)
        g_feat, g_coord = rng.standard_normal(tuple(ref.feat.shape)), rng.standard_normal(tuple(ref.coord.shape))
        torch.autograd.backward([ref.feat, ref.coord], [torch.from_numpy(g_feat), torch.from_numpy(g_coord)])
        ref_grads = [t.grad.numpy() for t in leaves64 + watched(m64)]
        results = {}
        for backend in ("hip", "torch"):
            p = point()
            leaves = [p.feat, p.coord]
            m.zero_grad()
            with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                out = with_backend(backend, lambda: U.upscale_module_forward(m, p))
            torch.autograd.backward([out.feat, out.coord], [dev(g_feat, out.feat.dtype), dev(g_coord, out.coord.dtype)])
            results[backend] = [out.feat.detach(), out.coord.detach()] + [t.grad.clone() for t in leaves + watched(m)]
        names = ["feat", "coord", "grad_feat", "grad_coord", "grad_skip_w", "grad_delta_x_w", "grad_delta_f_w", "grad_affine_w"]
        refs = [ref.feat.detach().numpy(), ref.coord.detach().numpy()] + ref_grads
        for what, a, b, r in zip(names, results["hip"], results["torch"], refs):
            pool.add(what, a, r, b)
    pool.settle(f"module/{'bf16_autocast' if autocast else 'f32'}")
