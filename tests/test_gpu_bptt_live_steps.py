"""The pair BPTT kernel (csrc/recurrent_pair.hip, the loop of models/decoderlstm.py:78-108 walked backwards) starts every caption
at its LAST LIVE step when the caller runs in live-row mode (dims.rows + decoder_prepare_rows, no dalphas, caphn_tune key 38 = 1):
above that step d logits, d Hs and the carried gradient are zero, so the kernel writes +0 into those rows of its per-step outputs
instead of computing them.  Key 38 = 0 is the kernel path without the table: every gradient must be equal bit for bit.

Shapes are the smallest the pair kernels accept; B = 5 leaves three idle workgroups in each half of the one group of eight.  "gru10"
(H = 10: halves of 8 and 2, no 16-byte alignment) takes the scalar form of the zero fill, the other two the 16-byte one."""
import dataclasses

import pytest
import torch

from oracle import caphn_oracle as O
from helpers import dec_dims, dec_params_from_oracle, maxdiff

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T, P, V = 5, 6, 5, 23
KEY = 38
CASES = {"gru": dict(H=12, cell="gru"), "lstm": dict(H=8, cell="lstm"), "gru10": dict(H=10, cell="gru")}
# one caption live on all T steps, one with a single live step, one with a hole (live at 0, 1, 4), one with no live target,
# one ordinary prefix; <pad> = 0 is the ignored target
CAPS = [[1, 7, 8, 9, 10, 2],
        [1, 0, 0, 0, 0, 0],
        [1, 7, 0, 0, 9, 0],
        [0, 0, 0, 0, 0, 0],
        [1, 7, 8, 2, 0, 0]]
LAST = [5, 0, 4, -1, 3]


@pytest.fixture(scope="module")
def ops():
    from caphn import ops as _ops
    return _ops


@pytest.fixture()
def lib():
    from caphn import _lib
    lib = _lib.load()
    lib.caphn_tune(13, V)                # deterministic gradients: bit for bit
    yield lib
    lib.caphn_tune(13, 0); lib.caphn_tune(KEY, 1)
    torch.cuda.synchronize()
    assert lib.caphn_device_error(1) == 0


_cache = {}


def _case(name):
    """Dims, parameters, batch and the oracle's gradients of one configuration: built once, never modified."""
    if name in _cache:
        return _cache[name]
    c = CASES[name]
    dims = O.Dims(D=10, F=8, E=8, H=c["H"], V=V, he=6, cell=c["cell"])
    p = O.init_params(dims, seed=11)
    feats = O.synth_batch(dims, B=B, T=T, P=P, seed=12)["features"]
    caps = torch.tensor(CAPS, dtype=torch.int64)
    x = torch.zeros(dims.he); x[1] = 1.0
    _, _, _, theta, gref = O.forward_backward(dims, p, x, feats, caps)
    dd = dataclasses.replace(dec_dims(dims, B, T, P), rows=True)
    params = dec_params_from_oracle(p, theta, dims, DEV)
    _cache[name] = (dims, dd, params, feats.to(DEV), caps.to(DEV), gref)
    return _cache[name]


def _regions(ops, dd, ws):
    return {w: ops.decoder_region(dd, ws, w) for w in (ops.REGION_DGI, ops.REGION_DGH, ops.REGION_DUAH, ops.REGION_DE)}


def _run(ops, lib, name, key, rows=True, dalphas=None, dlogits=None, poison=None):
    """prepare_rows, forward, cross entropy, backward on a fresh zeroed workspace and fresh zeroed gradients."""
    _, dd, params, feats, caps, _ = _case(name)
    dd = dataclasses.replace(dd, rows=rows)
    lib.caphn_tune(KEY, key)
    ws = ops.decoder_workspace(dd, DEV).zero_()
    ops.decoder_prepare_rows(dd, caps, 0, ws)           # (also without dims.rows: the table is there, the backward must not use it)
    logits = torch.full((B, T, V), 7.0, device=DEV)
    ops.decoder_forward(dd, params, feats, caps, ws, logits=logits)
    _, dl = ops.cross_entropy_fwd_bwd(logits, caps, 0)
    if dlogits is not None:
        dl = dlogits.clone()
    if poison == "outputs":
        for r in _regions(ops, dd, ws).values():
            r.fill_(float("nan"))
    elif poison == "skipped gates":
        gates = ops.decoder_region(dd, ws, ops.REGION_GATES)
        for b, l in enumerate(LAST):
            gates[b, l + 1:] = float("nan")
    grads = {n: torch.zeros(s, device=DEV) for n, s in dd.param_shapes().items()}
    ops.decoder_backward(dd, params, feats, caps, dl, grads, ws, dalphas=dalphas)
    torch.cuda.synchronize()
    return {"grads": grads, "regions": {w: r.clone() for w, r in _regions(ops, dd, ws).items()},
            "last": ops.decoder_region(dd, ws, ops.REGION_LAST_LIVE).clone()}


def _equal(a, b):
    return all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])


@pytest.mark.parametrize("name", list(CASES))
def test_equal_to_the_full_length_path(ops, lib, name):
    new, old = _run(ops, lib, name, 1), _run(ops, lib, name, 0)
    assert new["last"].tolist() == LAST
    for n in new["grads"]:
        assert bool(torch.isfinite(new["grads"][n]).all()), n
        assert torch.equal(new["grads"][n], old["grads"][n]), n        # (+0 == -0)
    assert any(float(g.abs().max()) > 0 for g in new["grads"].values())
    for w, r in new["regions"].items():
        for b, l in enumerate(LAST):
            assert float(r[b, l + 1:].abs().sum()) == 0.0, (w, b)       # exactly zero above each caption's start
            assert not bool(torch.signbit(r[b, l + 1:]).any()), (w, b)  # ... and +0, as written
        assert torch.equal(r, old["regions"][w]), w


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_oracle(ops, lib, name):
    dims, _, _, _, _, gref = _case(name)
    new = _run(ops, lib, name, 1)
    worst = {}
    for n, g in new["grads"].items():
        if not n.startswith(dims.cell + "."):
            worst[n] = maxdiff(g.cpu(), gref["captioner." + n])
    dth = torch.cat([new["grads"][dims.cell + "." + n].flatten() for n, _ in dims.cell_param_shapes()])
    worst["dtheta"] = maxdiff(dth.cpu(), gref["dtheta"])
    print(name, {n: "%.2e" % v for n, v in worst.items()})
    for n, v in worst.items():
        assert v < 1e-6, (n, v)


@pytest.mark.parametrize("name", list(CASES))
def test_gating_external_attention_gradient(ops, lib, name):
    """dalphas may be non-zero on padded steps: those steps then carry gradient and must be walked."""
    gen = torch.Generator().manual_seed(5)
    da = torch.randn(B, T, P, generator=gen).to(DEV)
    new, old = _run(ops, lib, name, 1, dalphas=da), _run(ops, lib, name, 0, dalphas=da)
    assert _equal(new, old)
    assert not _equal(new, _run(ops, lib, name, 1))
    # the padded steps were computed, not zero-filled: d e of the caption without any live target
    assert float(new["regions"][ops.REGION_DE][3].abs().max()) > 0


@pytest.mark.parametrize("name", list(CASES))
def test_gating_without_live_row_mode(ops, lib, name):
    """dims.rows = False: nothing promises zero d logits on ignored rows (here every row carries some)."""
    gen = torch.Generator().manual_seed(6)
    dl = (torch.randn(B, T, V, generator=gen) * 0.1).to(DEV)
    new, old = _run(ops, lib, name, 1, rows=False, dlogits=dl), _run(ops, lib, name, 0, rows=False, dlogits=dl)
    assert _equal(new, old)
    assert float(new["regions"][ops.REGION_DGI][3].abs().max()) > 0


@pytest.mark.parametrize("name", list(CASES))
def test_every_unvisited_row_is_written(ops, lib, name):
    """NaN in the four per-step output regions before the backward: whatever the kernel does not write reaches the GEMMs behind it."""
    ref = _run(ops, lib, name, 1)
    got = _run(ops, lib, name, 1, poison="outputs")
    for n in got["grads"]:
        assert bool(torch.isfinite(got["grads"][n]).all()), n
        assert torch.equal(got["grads"][n], ref["grads"][n]), n
    for w, r in got["regions"].items():
        assert bool(torch.isfinite(r).all()), w


@pytest.mark.parametrize("name", list(CASES))
def test_skipped_steps_are_not_walked(ops, lib, name):
    """NaN in the saved gate activations of the steps above each caption's start -- only the BPTT kernel reads them: the
    full-length walk multiplies them into every gradient, the shortened one never loads them."""
    ref = _run(ops, lib, name, 1)
    got = _run(ops, lib, name, 1, poison="skipped gates")
    for n in got["grads"]:
        assert torch.equal(got["grads"][n], ref["grads"][n]), n
    old = _run(ops, lib, name, 0, poison="skipped gates")
    assert not all(bool(torch.isfinite(g).all()) for g in old["grads"].values())
