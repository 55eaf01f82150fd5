"""UNet_Small trained from SymbolWindows (mural_indel_train_forward_symbols / _backward_symbols) against the dense route and the
reference's recorded step.

Bars.  The fixture comparison is the one tests/test_gpu_indel.py::test_train_step_matches_reference asserts for the dense route
(scores 1e-5 of their scale, loss 1e-5 relative, every gradient 2e-4 of (its tensor's max + 1e-2) with the conv-bias rule, running
statistics 1e-5); the symbol route is held to it against the fixture, and the symbol-versus-dense difference is held to the same bar
with the dense route in the fixture's place.  Nothing asks for bit-equality across the two routes: the symbol route's input unit sums
table entries where the dense route multiplies and adds, and its weight gradient sums in another order.

Measured on an MI355X, worst gradient (difference / bar) over all tensors, rev | norev:
  dense  vs fixture   0.659 (conv.1.bias)         | 0.533 (uplblocks.0.1.bias)
  symbol vs fixture   0.583 (conv.1.bias)         | 0.412 (uplblocks.0.1.bias)
  symbol vs dense     0.393 (uplblocks.0.1.bias)  | 0.258 (uplblocks.0.1.bias)
  symbol vs dense with dropout 0.1, same seed   0.413 | 0.168
  dense  vs dense (a second run from the same state)   0 | 0: at the fixtures' shape the dense route repeated bit for bit, so it has no
  run-to-run spread to record here; the symbol-versus-dense difference is rounding of the input unit, carried through the batch
  statistics of the layers behind it.
The loader-fed epochs and the graphed steps are held to the bar the repository already uses for two equivalent routes after a few
optimiser steps (tests/test_gpu_indel.py::test_graphed_indel_train_step_matches_eager: 1e-3 relative on the loss); measured: summed
loss of three steps 36.039728 (dense loader) vs 36.039710 (symbols=True), relative difference 5.0e-07; graphed last-step loss on uint8
input 4.7427483 against the eager symbol steps' 4.7427473, relative difference 2.0e-07."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from mural_amd import _lib
from tests import _loader_data as D
from tests import _util as U
from tests.test_gpu_indel import _train_step, product_from

pytestmark = pytest.mark.gpu


def to_symbols(x):
    B, _, L = x.shape
    sym = torch.empty((B, L), dtype=torch.uint8, device=x.device)
    status = torch.zeros(1, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().mural_op_dense_to_symbols(x.data_ptr(), B, L, sym.data_ptr(), status.data_ptr(), _lib.current_stream_ptr(x.device)))
    assert int(status.item()) == 0
    return sym


def _fresh(fx, p=0.0):
    orc = U.indel_oracle_from_hp(fx["hp"], fx["down"])
    m = product_from(fx)
    m.load_state_dict(U.indel_state_for(fx, orc), strict=True)
    m = m.cuda().train()
    m.out_fc[1].p = p
    return m


def _step(fx, x, p=0.0, seed=11):
    from mural_amd.data import SymbolWindows
    m = _fresh(fx, p)
    torch.manual_seed(seed)            # the dropout seed of the step is drawn from torch's CPU generator
    preds, loss = _train_step(m, SymbolWindows(x) if x.dtype is torch.uint8 else x, torch.from_numpy(fx["y"]).cuda())
    return dict(preds=preds.detach().cpu().numpy(), loss=float(loss.item()),
                grads={k: q.grad.cpu().numpy() for k, q in m.named_parameters()},
                bufs={k: b.cpu().numpy() for k, b in m.named_buffers()})


def _compare(got, want_preds, want_loss, want_grads, want_bufs, what):
    """The measure of test_train_step_matches_reference; returns the worst gradient (difference / bar) and its tensor."""
    assert np.abs(got["preds"] - want_preds).max() <= 1e-5 * max(1.0, float(np.abs(want_preds).max())), what
    assert abs(got["loss"] - want_loss) <= 1e-5 * abs(want_loss), what
    worst = (0.0, None)
    for k, g in got["grads"].items():
        want = want_grads[k]
        diff = float(np.abs(g - want).max())
        tol = 2e-4 * (np.abs(want).max() + 1e-2)
        if k.endswith(".bias") and k[:-4] + "weight" in want_grads and want.ndim == 1 and want_grads[k[:-4] + "weight"].ndim == 3:
            tol = max(tol, 2e-5 * np.abs(want_grads[k[:-4] + "weight"]).max())
        if diff / tol >= worst[0]:
            worst = (diff / tol, k)
        assert diff <= tol, (what, k, diff, tol)
    for k, b in got["bufs"].items():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(want_bufs[k]), (what, k)
        else:
            assert np.abs(b.astype(np.float64) - np.asarray(want_bufs[k], np.float64)).max() <= 1e-5, (what, k)
    print(f"[indel symbols] {what}: worst gradient difference / bar {worst[0]:.3g} at {worst[1]}")
    return worst


@pytest.mark.parametrize("tag", ["rev", "norev"])
def test_symbol_step_matches_dense_step_and_reference(tag):
    fx = U.load(f"indel_train_{tag}.npz")
    x = U.onehot(fx["codes"]).cuda()
    sym = to_symbols(x)
    fx_grads = {k[3:]: fx[k] for k in fx.files if k.startswith("g::")}
    fx_bufs = {k[3:]: fx[k] for k in fx.files if k.startswith("b::")}
    dense, dense2, symb = _step(fx, x), _step(fx, x), _step(fx, sym)
    _compare(dense, fx["preds"], float(fx["loss"]), fx_grads, fx_bufs, f"{tag} dense vs fixture")
    _compare(symb, fx["preds"], float(fx["loss"]), fx_grads, fx_bufs, f"{tag} symbols vs fixture")
    _compare(symb, dense["preds"], dense["loss"], dense["grads"], dense["bufs"], f"{tag} symbols vs dense")
    _compare(dense2, dense["preds"], dense["loss"], dense["grads"], dense["bufs"], f"{tag} dense vs dense (second run)")
    if tag == "rev":      # the strand-symmetrising BatchNorm is applied, and counted, twice (the fixture's counters start equal)
        assert int(symb["bufs"]["conv.1.num_batches_tracked"]) == int(symb["bufs"]["out_fc.0.num_batches_tracked"]) + 1
    # with dropout on: the same masks from the same seed in both routes
    dd, ds = _step(fx, x, p=0.1, seed=5), _step(fx, sym, p=0.1, seed=5)
    assert np.abs(dd["preds"] - dense["preds"]).max() > 1e-4        # (the masks did something)
    _compare(ds, dd["preds"], dd["loss"], dd["grads"], dd["bufs"], f"{tag} symbols vs dense, dropout 0.1")


def test_symbol_workspace_is_smaller_by_the_flipped_copy():
    from mural_amd.model.indel_train_step import _shape
    fx = U.load("indel_train_rev.npz")
    m = product_from(fx)
    B, L = fx["codes"].shape
    for b in (B, 128):
        shape = _shape(m, L)
        dense = int(_lib.lib().mural_indel_train_workspace_bytes(C.byref(shape), b))
        symb = int(_lib.lib().mural_indel_train_symbols_workspace_bytes(C.byref(shape), b))
        assert dense > 0 and symb > 0 and dense - symb >= b * 4 * L * 4, (b, dense, symb)
    bad = _shape(m, L + 1)
    assert int(_lib.lib().mural_indel_train_symbols_workspace_bytes(C.byref(bad), B)) == 0


def test_symbol_step_input_checks():
    from mural_amd.data import SymbolWindows
    fx = U.load("indel_train_rev.npz")
    m = _fresh(fx)
    sym = to_symbols(U.onehot(fx["codes"]).cuda())
    with pytest.raises(TypeError):
        m(SymbolWindows(sym.to(torch.int32)))
    with pytest.raises(ValueError):
        m(SymbolWindows(sym[:, :-1].contiguous()))      # a length the down_list does not admit


def test_eval_mode_takes_symbol_windows_bit_for_bit():
    from mural_amd.data import SymbolWindows
    for tag in ("rev", "norev"):
        fx = U.load(f"indel_train_{tag}.npz")
        m = _fresh(fx).eval()
        x = U.onehot(fx["codes"]).cuda()
        with torch.no_grad():
            a, b = m(x), m(SymbolWindows(to_symbols(x)))
        assert torch.equal(a, b), tag


# ------------------------------------------------------------------------------------------------ loader-fed epochs, graphed steps
DOWN = [1, 2, 5, 1, 1, 2]      # admits the fixture's window of 2 * 110 columns: 220 -> 220, 110, 22, 22, 22, 11
STEPS = 3


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return D.write_fixture(tmp_path_factory.mktemp("indel_symbols"))


def _loader(files, **kw):
    from mural_amd.data import EpochLoader
    return EpochLoader(*files, D.BATCH, D.R_LOCAL, D.ORDER, D.R_DISTAL, segment_center=D.SEGMENT, sampled_segments=D.SAMPLED,
                       model_type="indel", **kw)


def _model_and_optimizer():
    from mural_amd import train as TR
    from mural_amd.model import model_choice, weights_init
    config = dict(local_radius=D.R_LOCAL, local_order=D.ORDER, distal_radius=D.R_DISTAL, CNN_kernel_size=7, CNN_out_channels=8, down_list=DOWN,
                  use_reverse=True, n_class=4, model_no=0, optim="Adam", learning_rate=1e-3, weight_decay=1e-6, lr_scheduler="StepLR",
                  LR_gamma=0.9, batch_size=D.BATCH, min_lr=1e-7, restart_lr=1e-4)
    torch.manual_seed(0)
    m = model_choice(0, config, dict(n_class=4), "indel")
    m.apply(weights_init)
    m = m.cuda()
    m.out_fc[1].p = 0.0
    return m, TR.make_optimizer(config, m.parameters()), config


def test_loader_yields_symbol_windows_and_train_epoch_takes_them(files):
    from mural_amd import train as TR
    from mural_amd.data import SymbolWindows
    dense = list(_loader(files).epoch(shuffle=True, generator=torch.Generator().manual_seed(3)))
    symb = list(_loader(files, symbols=True).epoch(shuffle=True, generator=torch.Generator().manual_seed(3)))
    assert len(dense) == len(symb) > STEPS
    for (y0, _, cat0, x0), (y1, _, cat1, x1) in zip(dense, symb):
        assert isinstance(x1, SymbolWindows) and x1.sym.dtype == torch.uint8 and x0.dtype == torch.float32
        assert torch.equal(y0, y1) and torch.equal(cat0, cat1)
        assert torch.equal(x1.sym, to_symbols(x0))            # the same rows: integers, bit-exact
    with pytest.raises(ValueError):
        _loader(files, symbols=True, dense=True)
    losses = {}
    crit = torch.nn.CrossEntropyLoss(reduction="sum")
    for name, batches in (("dense", dense), ("symbols", symb)):
        m, opt, config = _model_and_optimizer()
        losses[name] = TR.train_epoch(m, itertools.islice(batches, STEPS), crit, opt, TR.make_scheduler(config, opt), config, "cuda",
                                      model_type="indel")
        assert int(m.conv[1].num_batches_tracked) == 2 * STEPS
    rel = abs(losses["symbols"] - losses["dense"]) / abs(losses["dense"])
    print(f"[indel symbols] train_epoch, {STEPS} steps: dense loader {losses['dense']!r}, symbols=True {losses['symbols']!r}, relative {rel:.3g}")
    assert np.isfinite(losses["symbols"]) and rel <= 1e-3


def test_graphed_step_on_uint8_input(files):
    """GraphedIndelTrainStep captured on a uint8 static input: the loss of its last replay against the same steps taken eagerly."""
    from mural_amd.data import SymbolWindows
    from mural_amd.train import GraphedIndelTrainStep
    y, _, _, x = next(iter(_loader(files, symbols=True).epoch(shuffle=False)))
    y = y.long().squeeze()
    crit = torch.nn.CrossEntropyLoss(reduction="sum")

    def make():
        m, _, _ = _model_and_optimizer()
        return m.train(), torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)

    eager, opt_e = make()
    for _ in range(3 + STEPS):            # the graphed step's 3 warm-up steps + STEPS replays
        _, loss = _train_step(eager, SymbolWindows(x.sym), y)
        torch.nn.utils.clip_grad_norm_(eager.parameters(), 10)
        opt_e.step()
    graphed, opt_g = make()
    step = GraphedIndelTrainStep(graphed, opt_g, crit, x.sym, y)
    assert step.x.dtype is torch.uint8
    for _ in range(STEPS):
        loss_g = step(x, y)               # SymbolWindows or the uint8 tensor itself
    step.finish()
    rel = abs(loss_g.item() - loss.item()) / abs(loss.item())
    print(f"[indel symbols] graphed on uint8: last loss {loss_g.item()!r}, eager {loss.item()!r}, relative {rel:.3g}")
    assert np.isfinite(loss_g.item()) and rel <= 1e-3
    assert int(graphed.conv[1].num_batches_tracked) == int(eager.conv[1].num_batches_tracked)
