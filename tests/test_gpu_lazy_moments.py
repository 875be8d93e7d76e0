"""Lazy moment write-back of the rank-1 Adam passes (caphn_rank_lag): m and v of a lagged member go back to
memory every K-th step only; the passes in between replay the pending steps from the saved gradient factors.  W, theta_next and
the settled moments must be bit-identical to the eager passes, at the kernel level and through FusedTrainer."""
import pytest
import torch

from helpers import TINY_DIMS, load_case, style_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def ops():
    from caphn import ops as _ops
    return _ops


def _up4(n):
    return (n + 3) & ~3


def _adam64(W, m, v, g, step):
    """torch.optim.Adam's single-tensor recurrence in float64 (the recurrence adam_elem implements in fp32)."""
    m.mul_(B1).add_(g, alpha=1 - B1)
    v.mul_(B2).addcmul_(g, g, value=1 - B2)
    denom = v.sqrt() / (1 - B2 ** step) ** 0.5 + EPS
    W.addcdiv_(m, denom, value=-LR / (1 - B1 ** step))


# (130, 260): k / 4 = 65 crosses the 64-lane boundary and the rows are no multiple of the row block; (33, 480): the k of head 0
@pytest.mark.parametrize("zero_gfac", [False, True], ids=["keep_gfac", "zero_gfac"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "next_theta"])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("rows,k", [(1, 4), (7, 20), (130, 260), (33, 480)])
def test_lagged_pass_equals_eager_bit_for_bit(ops, rows, k, K, fused, zero_gfac):
    """2K + 1 steps (two write-backs and a trailing partial cycle), a fresh rank-1 gradient and clip coefficient each step.
    After every step: W and theta_next equal the eager pass's, and a settle of the stale moments (on copies, so the cycle goes
    on) equals the eager moments -- that covers every phase of the cycle.  At the end the moments are settled in place.
    float64 reference: the same recurrence in double, bounds of tests/test_gpu_kernels.py's Adam tests (W 1e-6, m 1e-7, v 1e-9).
    W starts at N(0, 0.1^2), not N(0, 1): those bounds were set for two steps, and over nine steps the half-ulp rounding of a
    stored |W| in [2, 4) alone (1.2e-7 per step) can use them up -- the bound is meant for the update's arithmetic."""
    gen = torch.Generator().manual_seed(rows * 1000 + k * 10 + K)
    W0 = torch.randn(rows, k, generator=gen) * 0.1
    We, Wl = W0.to(DEV), W0.to(DEV)
    me, ve, ml, vl = (torch.zeros(rows, k, device=DEV) for _ in range(4))
    W64, m64, v64 = W0.double(), torch.zeros(rows, k, dtype=torch.float64), torch.zeros(rows, k, dtype=torch.float64)
    ring_row = torch.zeros(K - 1, _up4(rows), device=DEV)
    ring_col = torch.zeros(K - 1, _up4(k), device=DEV)
    nb = torch.randn(rows, generator=gen).to(DEV)
    the, thl = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    pending = 0
    for step in range(1, 2 * K + 2):
        gf = torch.randn(1, rows, generator=gen) * 1e-2
        af = torch.randn(1, k, generator=gen)
        c = float(torch.rand(1, generator=gen)) * 0.7 + 0.3
        coef = torch.tensor([c, 0.0], device=DEV)
        na = torch.randn(k, generator=gen).to(DEV)
        ge, gl, ad = gf.to(DEV), gf.to(DEV), af.to(DEV)
        kwe = dict(next_a=na, next_bias=nb, next_theta=the) if fused else {}
        kwl = dict(next_a=na, next_bias=nb, next_theta=thl) if fused else {}
        ops.adam_rank(We, me, ve, ge, ad, coef, LR, step, (B1, B2), EPS, zero_gfac=zero_gfac, **kwe)
        store = pending == K - 1
        lag = ops.rank_lag(pending, store, ring_row, ring_col, None if store else ring_row[pending],
                           None if store else ring_col[pending])
        ops.adam_rank(Wl, ml, vl, gl, ad, coef, LR, step, (B1, B2), EPS, zero_gfac=zero_gfac, lag=lag, **kwl)
        pending = 0 if store else pending + 1
        assert torch.equal(We, Wl), step
        if fused:
            assert torch.equal(the, thl), step
        assert torch.equal(gl, torch.zeros_like(gl) if zero_gfac else gf.to(DEV)), step
        if store:
            assert torch.equal(ml, me) and torch.equal(vl, ve), step
        else:       # mid-cycle: the moments in memory are stale by `pending` steps, a settle brings them up to date
            mc, vc = ml.clone(), vl.clone()
            ops.adam_rank_settle(mc, vc, (B1, B2), ops.rank_lag(pending, True, ring_row, ring_col))
            assert torch.equal(mc, me) and torch.equal(vc, ve), step
        g32 = (gf[0] * torch.tensor(c, dtype=torch.float32))            # gfac * coef is rounded to fp32 by the pass
        _adam64(W64, m64, v64, torch.outer(g32.double(), af[0].double()), step)
    assert pending == 1
    ops.adam_rank_settle(ml, vl, (B1, B2), ops.rank_lag(pending, True, ring_row, ring_col))
    assert torch.equal(ml, me) and torch.equal(vl, ve)
    dW, dm, dv = (float((a.double().cpu() - b).abs().max()) for a, b in ((Wl, W64), (ml, m64), (vl, v64)))
    print(f"max deviation from float64: W {dW:.3e} m {dm:.3e} v {dv:.3e}")
    assert dW < 1e-6 and dm < 1e-7 and dv < 1e-9


@pytest.mark.parametrize("case", ["k10", "offset4"])
def test_lagged_pass_refuses_shapes_of_the_other_kernels(ops, case):
    """k % 4 != 0 and a W that is only 4-byte aligned take the element-linear kernel in the eager pass; the lagged entry point
    returns CAPHN_EINVAL for them before it launches anything (nothing changes), and the eager call still works."""
    from caphn._lib import CaphnError
    gen = torch.Generator().manual_seed(5)
    rows, k = (12, 10) if case == "k10" else (12, 16)
    buf = (torch.randn(rows * k + 4, generator=gen) * 0.1).to(DEV)
    W = buf[1:1 + rows * k].view(rows, k) if case == "offset4" else buf[:rows * k].view(rows, k)
    assert W.data_ptr() % 16 == (4 if case == "offset4" else 0)
    m, v = torch.zeros(rows, k, device=DEV), torch.zeros(rows, k, device=DEV)
    gf, af = (torch.randn(1, rows, generator=gen) * 1e-2).to(DEV), torch.randn(1, k, generator=gen).to(DEV)
    coef = torch.tensor([0.5, 0.0], device=DEV)
    before = buf.clone()
    ring_row, ring_col = torch.zeros(1, _up4(rows), device=DEV), torch.zeros(1, _up4(k), device=DEV)
    for lag in (ops.rank_lag(0, True), ops.rank_lag(0, False, ring_row, ring_col, ring_row[0], ring_col[0])):
        with pytest.raises(CaphnError) as ei:
            ops.adam_rank(W, m, v, gf, af, coef, LR, 1, lag=lag)
        assert ei.value.rc == -1
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and not m.any() and not v.any() and not ring_row.any() and not ring_col.any()
    ops.adam_rank(W, m, v, gf, af, coef, LR, 1)
    assert not torch.equal(buf, before) and bool(m.any())


class _V:
    w2i = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "factual": 4}

    def __call__(self, w):
        return self.w2i.get(w, 3)


def _trainer(dims, p, g, cc):
    from hypernet_attention import HyperNet
    from models.decoderlstm import AttentionGru
    from caphn.engine import FusedTrainer
    net = HyperNet(dims.F, dims.E, dims.H, dims.V, _V(), cc=cc, hyper_emb=dims.he)
    net.captioner = AttentionGru(dims.D, dims.F, dims.E, dims.H, dims.V, p=0.0)
    net.load_state_dict(p, strict=False)
    tr = FusedTrainer(net.to(DEV), lr=1e-3, max_norm=float(g["clip_max_norm"]))
    tr.lazy_min_elems = 0          # the tiny heads are far below the default threshold: lag every head
    return tr


def _flat(tr):
    return torch.cat([tr.flat_p] + [w.data.flatten() for w in tr.W2])


def _sd_equal(a, b):
    assert a["param_names"] == b["param_names"] and len(a["state"]) == len(b["state"])
    for i in a["state"]:
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][i][key], b["state"][i][key]), (a["param_names"][i], key)


def test_trainer_with_lagged_heads_equals_eager_bit_for_bit():
    """gru_tiny_flickr in the deterministic-gradient mode: seven steps with K = 4 against seven with K = 1; a state_dict taken
    mid-cycle (after step 2); a trainer restored from such a checkpoint (with a pending step of its own, which the load drops) and
    stepped five more times against the uninterrupted one; step_graphed calls (eager first call, capture, replay) after three lagged steps."""
    from caphn import _lib
    lib = _lib.load()
    name = "gru_tiny_flickr"
    dims = TINY_DIMS[name]
    g, p = load_case(name)
    x, tok = style_args(g)
    cc = tok is None
    feats, caps = g["features"].to(DEV), g["captions"].to(DEV)
    kw = dict(style_token=tok, next_style_token=tok) if tok is not None else dict(x_style=x.to(DEV))
    gkw = dict(style_token=tok) if tok is not None else dict(x_style=x.to(DEV))
    K0 = lib.caphn_lazy_moments_period()

    def run(K):
        assert lib.caphn_tune(37, K) == 0
        out = {}
        a = _trainer(dims, p, g, cc)
        for _ in range(2):
            a.step(feats, caps, **kw)
        if K > 1:
            assert any(st.pending for st in a._lag.values())          # really mid-cycle
        out["sd2"] = a.state_dict()
        out["model2"] = {k_: v_.detach().cpu().clone() for k_, v_ in a.net.state_dict().items()}
        for _ in range(5):
            a.step(feats, caps, **kw)
        out["p7"] = _flat(a).clone()
        out["sd7"] = a.state_dict()
        if K > 1:
            assert sorted(a._lag) == list(range(len(a.W2))) and not any(st.refused for st in a._lag.values())
        # resume against the uninterrupted run, WITHOUT the announced next style: a resumed trainer computes its first theta with
        # the forward GEMV, an uninterrupted one takes it from the previous Adam pass's fused GEMV (another summation order),
        # so only without that prefetch are the two runs the same arithmetic
        u = _trainer(dims, p, g, cc)
        for _ in range(2):
            u.step(feats, caps, **gkw)
        ck_opt = u.state_dict()
        ck_model = {k_: v_.detach().cpu().clone() for k_, v_ in u.net.state_dict().items()}
        for _ in range(5):
            u.step(feats, caps, **gkw)
        out["u7"] = _flat(u).clone()
        out["usd7"] = u.state_dict()
        c = _trainer(dims, p, g, cc)
        c.step(feats, caps, **gkw)                 # a trainer that already ran: one lagged step pending, which the load drops
        if K > 1:
            assert any(st.pending for st in c._lag.values())
        c.net.load_state_dict(ck_model, strict=False)
        c.load_state_dict(ck_opt)
        assert not any(st.pending for st in c._lag.values())
        for _ in range(5):
            c.step(feats, caps, **gkw)
        out["c7"] = _flat(c).clone()
        out["csd7"] = c.state_dict()
        b = _trainer(dims, p, g, cc)
        for _ in range(3):
            b.step(feats, caps, **kw)
        out["graphed"] = []
        for _ in range(3):                         # first call with a key runs eagerly, the second captures, the third replays
            b.step_graphed(feats, caps, **gkw)
            out["graphed"].append(_flat(b).clone())
        out["gsd"] = b.state_dict()
        return out

    try:
        assert lib.caphn_tune(13, dims.V) == 0
        e, l = run(1), run(4)
    finally:
        assert lib.caphn_tune(13, 0) == 0
        assert lib.caphn_tune(37, K0) == 0
    _sd_equal(e["sd2"], l["sd2"])
    assert torch.equal(e["p7"], l["p7"])
    _sd_equal(e["sd7"], l["sd7"])
    print("resumed - uninterrupted, max abs: eager %.3e lagged %.3e" % (float((e["c7"] - e["u7"]).abs().max()),
                                                                       float((l["c7"] - l["u7"]).abs().max())))
    assert torch.equal(e["u7"], l["u7"]) and torch.equal(l["c7"], l["u7"]) and torch.equal(e["c7"], l["c7"])
    _sd_equal(l["usd7"], l["csd7"])
    _sd_equal(e["usd7"], l["usd7"])
    for pe, pl in zip(e["graphed"], l["graphed"]):
        assert torch.equal(pe, pl)
    _sd_equal(e["gsd"], l["gsd"])
