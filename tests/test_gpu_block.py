"""GPU: the fused residual junctions of the decoder Block (csrc/block.hip through generativedensification_amd.block) against the
float64 restatement (tests/block_ref.py) and against the torch composition on the same GPU in the same dtypes, and the bound
forward against the "torch" backend and a float64 copy of the module.

Accuracy bar, for every output and gradient: with e_hip = max|hip - ref64| and e_torch = max|torch - ref64| (ref64 on the inputs
as rounded to their dtypes), e_hip <= 2 e_torch + half an ulp of the result dtype at max|ref64|.  The maxima are pooled over the
draws of a case (tests/block_cases.py: every judged tensor has at least 256 elements in all); every pooled pair is printed
before it is asserted.

Bit identities pin the instruction sequence: n of an ada `post` is norm.ada_layer_norm(y, scale, offset), n of a plain LN is
norm.ada_layer_norm(y, ones, offset), and two calls are bitwise equal, forward and backward."""
import copy

import numpy as np
import pytest
import torch

import block_cases as BC
import block_ref as R

pytestmark = pytest.mark.gpu
point_of = R.point_of

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

# dtype sets: name -> (dtype of branch / keep / ada scale, of skip and LN weight / bias, autocast).  The trainer's set runs under
# bf16 autocast with a float32 skip and a bf16 branch, as the Block meets them behind a Linear.
SETS = {"f32": (F32, F32, False), "bf16": (BF16, BF16, False), "f16": (F16, F16, False), "trainer": (BF16, F32, True)}


def block():
    from generativedensification_amd import block as B

    return B


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

    def add(self, what, hip, ref, tor):
        assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape, ref.shape)
        assert np.isfinite(f64(hip)).all(), what
        row = self.rows.setdefault(what, [0.0, 0.0, 0.0, hip.dtype, 0])
        if ref.size:
            row[0] = max(row[0], float(np.abs(f64(hip) - ref).max()))
            row[1] = max(row[1], float(np.abs(f64(tor) - ref).max()))
            row[2] = max(row[2], float(np.abs(ref).max()))
        row[4] += ref.size

    def settle(self, tag):
        bad = []
        for what, (e_hip, e_torch, mag, dtype, count) in self.rows.items():
            slack = R.half_ulp(dtype, mag)
            print(f"block-bar {tag}/{what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e} elements={count}")
            assert count >= 256, (what, count)
            if not e_hip <= 2 * e_torch + slack:
                bad.append((what, e_hip, e_torch, slack))
        assert not bad, bad


# ---- the junction ---------------------------------------------------------------------------------------------------------

def spec_on_device(spec, lo, hi):
    """the numpy spec on the device (ada scale in `lo`, LN weight / bias in `hi`) -> (spec of detached tensors, spec as float64)"""
    if spec is None:
        return None, None
    parts = [None if p is None else dev(p, lo if spec[0] == "ada" else hi) for p in spec[1:-1]]
    return (spec[0], *parts, spec[-1]), (spec[0], *[None if p is None else f64(p) for p in parts], spec[-1])


def with_leaves(spec):
    if spec is None:
        return None, []
    leaves = [None if p is None else leaf(p) for p in spec[1:-1]]
    return (spec[0], *leaves, spec[-1]), leaves


def junction_once(name, set_name, draw, pool):
    B = block()
    lo, hi, autocast = SETS[set_name]
    skip64, branch64, keep64, pre64, post64, offset, gy64, gn64 = BC.inputs(name, draw)
    skip, branch = dev(skip64, hi), dev(branch64, lo)
    keep = None if keep64 is None else (dev(keep64, lo) if draw % 2 == 0 else dev(keep64, lo).reshape(-1, 1))      # (N,) and (N, 1)
    off = dev(offset)
    pre, r_pre = spec_on_device(pre64, lo, hi)
    post, r_post = spec_on_device(post64, lo, hi)
    runs = []
    for fn in (B.junction, R.torch_junction):
        a, b = leaf(skip), leaf(branch)
        s_pre, l_pre = with_leaves(pre)
        s_post, l_post = with_leaves(post)
        with torch.autocast("cuda", dtype=BF16, enabled=autocast):
            y, n = fn(a, b, keep, s_pre, s_post, off)
        runs.append((y, n, [a, b] + (l_pre + [None, None])[:2] + (l_post + [None, None])[:2]))
    (y, n, leaves), (ty, tn, t_leaves) = runs
    assert y.dtype == ty.dtype and y.is_contiguous() and (n is None) == (tn is None) == (post is None)
    gy = dev(gy64, y.dtype)
    outs, t_outs, gs = [y], [ty], [gy]
    if n is not None:
        assert n.dtype == tn.dtype and n.is_contiguous()
        gn = dev(gn64, n.dtype)
        outs, t_outs, gs = [y, n], [ty, tn], [gy, gn]
    torch.autograd.backward(outs, gs)
    torch.autograd.backward(t_outs, gs)
    r = (f64(skip), f64(branch), None if keep is None else f64(keep).reshape(-1))
    ref_y, ref_n = R.junction(*r, r_pre, r_post, offset)
    pool.add("y", y, ref_y, ty)
    if n is not None:
        pool.add("n", n, ref_n, tn)
    want = R.junction_grad(*r, r_pre, r_post, offset, f64(gy), f64(gs[1]) if n is not None else None)
    for what, a, b in zip(("skip", "branch", "pre_w", "pre_b", "post_w", "post_b"), leaves, t_leaves):
        assert (a is None) == (want[what] is None), what
        if a is not None:
            assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
            pool.add("grad_" + what, a.grad, want[what], b.grad)
    # rows at or behind the last end are zero through an ada norm; an empty segment gets a zero scale gradient
    seg = np.searchsorted(offset, np.arange(skip.shape[0]), side="right")
    tail = torch.as_tensor(seg >= len(offset)).to(DEV)
    empty = torch.as_tensor(np.bincount(seg, minlength=len(offset) + 1)[:len(offset)] == 0).to(DEV)
    if post is not None and post[0] == "ada":
        assert not n[tail].any() and not leaves[4].grad[empty].any()
    if pre is not None and pre[0] == "ada":
        assert torch.equal(y[tail], skip[tail].to(y.dtype)) and not leaves[1].grad[tail].any() and not leaves[2].grad[empty].any()
    return [y] + ([n] if n is not None else []) + [t.grad for t in leaves if t is not None]


def run_junction(name, set_name):
    pool = Pool()
    for draw in range(BC.draws(name)):
        junction_once(name, set_name, draw, pool)
    pool.settle(f"junction/{name}/{set_name}")


@pytest.mark.parametrize("name", list(BC.CASES))
def test_junction_f32_at_every_shape(name):
    run_junction(name, "f32")


@pytest.mark.parametrize("set_name", ["bf16", "f16", "trainer"])
@pytest.mark.parametrize("name", BC.DTYPE_CASES)
def test_junction_16_bit_and_the_autocast_mix(name, set_name):
    run_junction(name, set_name)


@pytest.mark.parametrize("set_name", ["f32", "bf16", "trainer"])
@pytest.mark.parametrize("name", ["j1_ada_c160_n70", "j2_ada_c40_n70", "j2_ada_c256_n33", "j1_ln_c8_n70", "j1_ln_c520_n7", "j2_ln_c256_n7",
                                  "j2_ln_c160_n70_nokeep"])
def test_post_norm_is_ada_layer_norm_bitwise(name, set_name):
    """n is norm.ada_layer_norm at the y the call returned: with the scale for an ada post, with ones for a plain LN (whose
    segments then end at N: a plain LN has no rows behind an end)"""
    B, N = block(), norm()
    lo, hi, autocast = SETS[set_name]
    skip64, branch64, keep64, pre64, post64, offset, _, _ = BC.inputs(name)
    skip, branch, keep, off = dev(skip64, hi), dev(branch64, lo), None if keep64 is None else dev(keep64, lo), dev(offset)
    pre, post = spec_on_device(pre64, lo, hi)[0], spec_on_device(post64, lo, hi)[0]
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        y, n = B.junction(skip, branch, keep, pre, post, off)
        if post[0] == "ada":
            want = N.ada_layer_norm(y, post[1], off, post[2])
        else:
            want = N.ada_layer_norm(y, torch.ones(1, y.shape[1], dtype=y.dtype, device=DEV), dev(np.array([y.shape[0]])), post[3])
    assert n.dtype == want.dtype and torch.equal(n, want), float((n.float() - want.float()).abs().max())


def test_two_calls_are_bitwise_equal():
    runs = [junction_once("mixed_c160_n70", "trainer", 0, Pool()) + junction_once("j1_affine_c40_n33", "f32", 1, Pool())
            + junction_once("j2_ada_c40_n70", "bf16", 0, Pool()) for _ in range(2)]
    assert len(runs[0]) == len(runs[1]) >= 16
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def guarded(rows, cols, dtype, fill=7.0, guard=16):
    full = torch.full((rows + 2 * guard, cols), fill, dtype=dtype, device=DEV)
    return full, full[guard:guard + rows]


def guards_kept(full, rows, fill=7.0, guard=16):
    return bool((full[:guard] == fill).all()) and bool((full[guard + rows:] == fill).all())


def test_guard_rows_round_every_output_keep_their_fill():
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M

    B = block()
    lib = L.load()
    dt = {F32: L.GDR_NORM_DTYPES["f32"], BF16: L.GDR_NORM_DTYPES["bf16"]}
    rng = np.random.default_rng(5)
    n, c, off_np = 70, 40, np.array([40, 40, 66])
    skip, branch = dev(rng.standard_normal((n, c)), F32), dev(rng.standard_normal((n, c)), BF16)
    keep, off = dev((rng.uniform(size=n) < 0.7) / 0.7, BF16), dev(off_np)
    scale, w, bias = dev(rng.standard_normal((3, c)), F32), dev(1 + 0.3 * rng.standard_normal(c), F32), dev(rng.standard_normal(c), F32)

    def descs(gs=None, gw=None, gb=None):
        pre, post = L.GdrBlockNorm(), L.GdrBlockNorm()
        pre.kind, pre.eps, pre.w, pre.w_dtype, pre.w_stride = L.GDR_BLOCK_NORM_ADA, 1e-5, scale.data_ptr(), dt[F32], c
        post.kind, post.eps, post.w, post.w_dtype, post.b, post.b_dtype = L.GDR_BLOCK_NORM_LN_AFFINE, 1e-5, w.data_ptr(), dt[F32], bias.data_ptr(), dt[F32]
        if gs is not None:
            pre.grad_w, post.grad_w, post.grad_b = gs.data_ptr(), gw.data_ptr(), gb.data_ptr()
        return pre, post

    y_full, y = guarded(n, c, F32)
    n_full, nn_ = guarded(n, c, F32)
    pre, post = descs()
    L.check(lib.gdr_block_junction_forward(skip.data_ptr(), c, dt[F32], branch.data_ptr(), c, dt[BF16], keep.data_ptr(), dt[BF16], pre, post,
                                           off.data_ptr(), n, 3, c, dt[F32], dt[F32], y.data_ptr(), dt[F32], nn_.data_ptr(), dt[F32], M.stream()),
            "junction_forward")
    gs_full, gs = guarded(n, c, F32)
    gb_full, gb = guarded(n, c, BF16)
    gsc_full, gsc = guarded(3, c, F32)
    gw_full, gw = guarded(1, c, F32)
    gbi_full, gbi = guarded(1, c, F32)
    gy, gn = dev(rng.standard_normal((n, c)), F32), dev(rng.standard_normal((n, c)), F32)
    nbytes = lib.gdr_block_junction_backward_bytes(n, 3, c)
    assert nbytes > 0
    ws, base, usable = M.workspace(nbytes, DEV)
    pre, post = descs(gsc, gw, gbi)
    L.check(lib.gdr_block_junction_backward(gy.data_ptr(), c, dt[F32], gn.data_ptr(), c, dt[F32], skip.data_ptr(), c, dt[F32], branch.data_ptr(), c,
                                            dt[BF16], keep.data_ptr(), dt[BF16], pre, post, off.data_ptr(), n, 3, c, dt[F32], dt[F32], dt[F32],
                                            base, usable, gs.data_ptr(), gb.data_ptr(), M.stream()), "junction_backward")
    torch.cuda.synchronize()
    assert guards_kept(y_full, n) and guards_kept(n_full, n) and guards_kept(gs_full, n) and guards_kept(gb_full, n)
    assert guards_kept(gsc_full, 3) and guards_kept(gw_full, 1) and guards_kept(gbi_full, 1)
    # (written whole: the float32 outputs hold no fill; the bf16 grad_branch is compared with the public call below)
    assert not (y == 7.0).any() and not (nn_ == 7.0).any() and not (gs == 7.0).any()
    assert not (gsc == 7.0).any() and not (gw == 7.0).any() and not (gbi == 7.0).any()
    assert not gb[66:].any() and not gsc[1].any() and torch.equal(y[66:], skip[66:])
    a, b, s, ww, bb = leaf(skip), leaf(branch), leaf(scale), leaf(w), leaf(bias)
    want = B.junction(a, b, keep, ("ada", s, 1e-5), ("ln", ww, bb, 1e-5), off)
    assert torch.equal(y, want[0]) and torch.equal(nn_, want[1])
    torch.autograd.backward(list(want), [gy, gn])
    assert torch.equal(gs, a.grad) and torch.equal(gb, b.grad) and torch.equal(gsc, s.grad) and torch.equal(gw[0], ww.grad) and torch.equal(gbi[0], bb.grad)


def test_unneeded_gradients_are_not_stored_and_none_gradients_read_as_zeros(monkeypatch):
    B = block()
    from generativedensification_amd import _lib as L

    lib = L.load()
    seen = []
    real = lib.gdr_block_junction_backward

    def spy(*args):
        pre, post = args[14], args[15]
        seen.append((args[0], args[3], args[-3], args[-2], pre.grad_w if pre is not None else None, post.grad_w, post.grad_b))
        return real(*args)

    skip64, branch64, keep64, pre64, post64, offset, gy64, gn64 = BC.inputs("mixed_c160_n70")
    skip, branch, keep, off, gy, gn = dev(skip64, F32), dev(branch64, F32), dev(keep64, F32), dev(offset), dev(gy64, F32), dev(gn64, F32)
    pre, post = spec_on_device(pre64, F32, F32)[0], spec_on_device(post64, F32, F32)[0]
    full = [leaf(skip), leaf(branch), leaf(pre[1]), leaf(post[1]), leaf(post[2])]
    torch.autograd.backward(list(B.junction(full[0], full[1], keep, ("ada", full[2], pre[2]), ("ln", full[3], full[4], post[3]), off)), [gy, gn])
    monkeypatch.setattr(lib, "gdr_block_junction_backward", spy)
    for i in range(5):
        ins = [skip, branch, pre[1], post[1], post[2]]
        ins[i] = leaf(ins[i])
        torch.autograd.backward(list(B.junction(ins[0], ins[1], keep, ("ada", ins[2], pre[2]), ("ln", ins[3], ins[4], post[3]), off)), [gy, gn])
        assert [o is not None for o in seen[-1][2:]] == [j == i for j in range(5)], (i, seen[-1])
        assert torch.equal(ins[i].grad, full[i].grad), i
    # only y is used: grad_n reaches the kernel as NULL and reads as zeros; only n: grad_y is NULL
    r = (f64(skip), f64(branch), f64(keep))
    r_pre, r_post = ("ada", f64(pre[1]), pre[2]), ("ln", f64(post[1]), f64(post[2]), post[3])
    for use_y in (True, False):
        a, b = leaf(skip), leaf(branch)
        y, n = B.junction(a, b, keep, pre, post, off)
        (y if use_y else n).backward(gy if use_y else gn)
        assert (seen[-1][0] is not None, seen[-1][1] is not None) == (use_y, not use_y)
        want = R.junction_grad(*r, r_pre, r_post, offset, f64(gy) if use_y else None, None if use_y else f64(gn))
        for got, w in ((a.grad, want["skip"]), (b.grad, want["branch"])):
            assert np.abs(f64(got) - w).max() <= 1e-5 * max(1.0, np.abs(w).max())


def test_no_host_synchronisation():
    B = block()
    skip64, branch64, keep64, pre64, post64, offset, gy64, gn64 = BC.inputs("mixed_c160_n70")
    skip, branch, keep, off = dev(skip64, F32), dev(branch64, BF16), dev(keep64, BF16), dev(offset)
    pre, post = spec_on_device(pre64, BF16, F32)[0], spec_on_device(post64, BF16, F32)[0]

    def call():
        a, b = leaf(skip), leaf(branch)
        s_pre, l_pre = with_leaves(pre)
        s_post, l_post = with_leaves(post)
        with torch.autocast("cuda", dtype=BF16):
            y, n = B.junction(a, b, keep, s_pre, s_post, off)
        (y.sum() + n.sum()).backward()
        return [y, n, a.grad, b.grad] + [t.grad for t in l_pre + l_post]

    want = call()                                        # warm-up: library load, kernel images
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            off[-1].item()                               # the canary: a read-back
        except RuntimeError:
            raised = True
        if raised:
            got = call()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_result_dtypes_are_the_compositions_and_empty_inputs_return_empty_tensors(monkeypatch):
    B = block()
    skip64, branch64, keep64, pre64, post64, offset, _, _ = BC.inputs("mixed_c160_n70")
    off = dev(offset)
    for autocast in (False, True):
        for lo, hi in ((F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)):
            if not autocast and lo != hi:
                specs = [(None, ("ln", None, None, 1e-5)), (None, None), (("ln", None, None, 1e-5), ("ada", dev(pre64[1], lo), 1e-5))]
            else:
                specs = [(spec_on_device(pre64, lo, hi)[0], spec_on_device(post64, lo, hi)[0]), (None, ("ln", None, None, 1e-5)), (None, None)]
            for pre, post in specs:
                with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                    got = B.junction(dev(skip64, hi), dev(branch64, lo), dev(keep64, lo), pre, post, off)
                    want = R.torch_junction(dev(skip64, hi), dev(branch64, lo), dev(keep64, lo), pre, post, off)
                assert got[0].dtype == want[0].dtype and (got[1] is None) == (want[1] is None), (autocast, lo, hi)
                if got[1] is not None:
                    assert got[1].dtype == want[1].dtype, (autocast, lo, hi, got[1].dtype, want[1].dtype)
                    if autocast:
                        assert got[1].dtype == F32
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    z = lambda *shape, dtype=F32: torch.zeros(*shape, dtype=dtype, device=DEV)      # noqa: E731
    y, n = B.junction(z(0, 16), z(0, 16, dtype=BF16), None, None, ("ada", z(2, 16), 1e-5), torch.tensor([0, 0], device=DEV))
    assert y.shape == n.shape == (0, 16) and y.dtype == n.dtype == F32
    y, n = B.junction(z(0, 16, dtype=BF16), z(0, 16, dtype=BF16))
    assert y.shape == (0, 16) and y.dtype == BF16 and n is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.junction(z(4, 16), z(4, 16), None, None, ("ada", z(1, 16), 1e-5), torch.tensor([4]))


# ---- the bound forward ----------------------------------------------------------------------------------------------------

KERNELS = ("gdr_block_junction_forward", "gdr_block_junction_backward")
COUNTS = (48, 48)       # 96 points in two segments
WATCHED = {"ln": ["cpe.0.weight", "cpe.1.weight", "attn.qkv.weight", "attn.proj.weight", "mlp.0.fc1.weight", "mlp.0.fc2.weight"],
           "ada": ["cpe.0.weight", "cpe.1.weight", "cpe.2.affine.weight", "norm1.0.affine.weight", "attn.qkv.weight", "norm2.0.affine.weight",
                   "mlp.0.fc2.weight"]}


def gpu_block(kind, drop_path, seed):
    from generativedensification_amd import serattn as S

    m = R.make_block(16, 2, 8, norm=kind, conv="hip", drop_path=drop_path, seed=seed, ada_forward=norm().ada_layer_norm_forward,
                     attn_forward=S.serialized_attention_forward)
    return m.to(DEV)


def with_backend(name, fn):
    B = block()
    old = B.BLOCK_BACKEND
    B.BLOCK_BACKEND = name
    try:
        return fn()
    finally:
        B.BLOCK_BACKEND = old


def counting(counts, name, real):
    def call(*args):
        counts[name] += 1
        return real(*args)

    return call


class Replay(torch.nn.Module):
    """multiplies by the recorded drop-path tensors in turn: the float64 copy sees the draws of the run it judges"""

    def __init__(self, keeps):
        super().__init__()
        self.keeps = list(keeps)

    def forward(self, x):
        return x * self.keeps.pop(0).double().cpu()


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16_autocast"])
@pytest.mark.parametrize("kind", ["ln", "ada"])
def test_bound_forward_meets_the_bar_beside_the_torch_backend(kind, autocast, training, monkeypatch):
    """both backends against a float64 copy of the module (table conv, restated attention, the run's own drop-path draws); the
    hip backend launches exactly the three junctions each way and none of the lines it replaces; a seeded run leaves the
    generator where the torch backend leaves it"""
    B = block()
    from generativedensification_amd import _lib as L
    from generativedensification_amd import upscale as U

    lib = L.load()
    pool = Pool()
    for seed in range(2):
        m = gpu_block(kind, 0.3 if training else 0.0, seed)
        m.train(training)
        type(m).forward = B.block_forward                   # the binding, on the stand-in's class
        assert B.covers(m)
        data = BC.block_point(COUNTS, 16, seed=seed)
        rng = np.random.default_rng(seed)
        g64 = rng.standard_normal((sum(COUNTS), 16))
        results, states, keeps = {}, {}, []
        real_keep = U._keep_tensor

        def recording(drop_path, branch):
            keep = real_keep(drop_path, branch)
            keeps.append(keep)
            return keep

        for backend in ("hip", "torch"):
            p = point_of(data, F32, DEV, grad=True)
            x = p.feat
            m.zero_grad()
            torch.manual_seed(7)
            counts = dict.fromkeys(KERNELS, 0)
            with monkeypatch.context() as mp:
                if backend == "hip":
                    for k in KERNELS:
                        mp.setattr(lib, k, counting(counts, k, getattr(lib, k)))
                    mp.setattr(U, "_keep_tensor", recording)

                    def boom(*a, **kw):
                        raise AssertionError("a torch fall-back ran in the HIP path")

                    fallbacks = [(B, "_reference_forward"), (torch.nn.LayerNorm, "forward"), (type(m.norm1[0]), "forward")]
                    if training:
                        fallbacks.append((type(m.drop_path[0]), "forward"))
                    for obj, attr in fallbacks:
                        mp.setattr(obj, attr, boom)
                with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                    out = with_backend(backend, lambda: m(p))
                states[backend] = torch.cuda.get_rng_state(DEV)
                assert out.feat is out.sparse_conv_feat.features and out.feat.dtype == F32 and "stem" in out.sparse_conv_feat.indice_dict
                out.feat.backward(dev(g64, F32))
            if backend == "hip":
                assert counts == dict.fromkeys(KERNELS, 3), counts
            params = dict(m.named_parameters())
            results[backend] = [out.feat.detach(), x.grad.clone()] + [params[k].grad.clone() for k in WATCHED[kind]]
        assert torch.equal(states["hip"], states["torch"])
        if training:
            assert len(keeps) == 2 and all((k == 0).any() and not (k == 0).all() for k in keeps)
        else:
            assert keeps == [None, None]
        # the float64 copy
        m64 = R.make_block(16, 2, 8, norm=kind, conv="table", seed=seed).double()
        m64.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()}, strict=True)
        if training:
            m64.drop_path = type(m64.drop_path)(Replay(keeps))
        p64 = point_of(data, torch.float64, "cpu", grad=True)
        x64 = p64.feat
        ref = R.restated_forward(m64, p64)
        ref.feat.backward(torch.from_numpy(g64))
        params64 = dict(m64.named_parameters())
        refs = [ref.feat.detach().numpy(), x64.grad.numpy()] + [params64[k].grad.numpy() for k in WATCHED[kind]]
        for what, a, b, r in zip(["feat", "grad_feat"] + ["grad_" + k for k in WATCHED[kind]], results["hip"], results["torch"], refs):
            pool.add(what, a, r, b)
    pool.settle(f"block/{kind}/{'bf16_autocast' if autocast else 'f32'}/{'train' if training else 'eval'}")


@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16_autocast"])
@pytest.mark.parametrize("kind", R.RECORDS)
def test_bound_forward_meets_the_bar_against_the_reference_blocks_record(kind, autocast):
    """the recorded run of the reference's own Block (tests/golden/block_<kind>.npz, float64) is the truth here, not a copy of the
    module made by this project: the record's state_dict under strict=True, its point, its upstream gradient; both backends over
    the drop-ins; the output, the input gradient and every parameter gradient of at least 256 elements (the weight matrices: a
    single record has one draw, and the CPU test holds the smaller ones to 1e-12) under the bar"""
    B = block()
    from generativedensification_amd import serattn as S

    rec = R.load_record(kind)
    m = R.block_of_record(rec, conv="hip", ada_forward=norm().ada_layer_norm_forward, attn_forward=S.serialized_attention_forward)
    m = m.float().to(DEV)
    type(m).forward = B.block_forward
    assert B.covers(m) and not m.training
    watched = [k for k, v in rec["gparam"].items() if v.size >= 256]
    assert {"cpe.0.weight", "cpe.1.weight", "attn.qkv.weight", "attn.proj.weight", "mlp.0.fc1.weight", "mlp.0.fc2.weight"} <= set(watched)
    assert ("norm1.0.affine.weight" in watched) == (kind == "ada")
    results = {}
    for backend in ("hip", "torch"):
        p = point_of(rec["data"], F32, DEV, grad=True)
        x = p.feat
        m.zero_grad()
        with torch.autocast("cuda", dtype=BF16, enabled=autocast):
            out = with_backend(backend, lambda: m(p))
        assert out.feat is out.sparse_conv_feat.features and out.feat.dtype == F32
        out.feat.backward(dev(rec["up"], F32))
        params = dict(m.named_parameters())
        results[backend] = [out.feat.detach(), x.grad.clone()] + [params[k].grad.clone() for k in watched]
    refs = [rec["out"], rec["gin"]["feat"]] + [rec["gparam"][k] for k in watched]
    pool = Pool()
    for what, a, b, r in zip(["feat", "grad_feat"] + ["grad_" + k for k in watched], results["hip"], results["torch"], refs):
        pool.add(what, a, r, b)
    pool.settle(f"block-record/{kind}/{'bf16_autocast' if autocast else 'f32'}")


def test_outside_covers_the_hip_backend_runs_the_reference_lines():
    B = block()
    m = gpu_block("ln", 0.0, 0)
    m.eval()
    data = BC.block_point(COUNTS, 16)
    want = with_backend("torch", lambda: B.block_forward(m, point_of(data, F32, DEV)))
    m.mlp[0].act = torch.nn.ReLU()
    assert not B.covers(m)
    a = with_backend("torch", lambda: B.block_forward(m, point_of(data, F32, DEV)))
    b = with_backend("hip", lambda: B.block_forward(m, point_of(data, F32, DEV)))
    assert torch.equal(a.feat, b.feat) and not torch.equal(a.feat, want.feat)
    assert m.cpe[0].training                                  # the reference's quirk: the conv is put into training mode
    copy.deepcopy(m)
