"""Run by tests/test_product_indel_symbols.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: one INDEL training step from SymbolWindows
through the product library (libmural_hip.so) -- the symbol entries resolve there and give the dense route's scores and gradients."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from mural_amd import _lib
    from mural_amd.data import SymbolWindows
    from tests import _util as U
    from tests.test_gpu_indel import _train_step, product_from
    assert _lib.flavor() == "product"
    for name in ("mural_indel_train_forward_symbols", "mural_indel_train_backward_symbols", "mural_op_indel_first_fwd"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib()._name == _lib.LIB_PATH
    fx = U.load("indel_train_rev.npz")
    orc = U.indel_oracle_from_hp(fx["hp"], fx["down"])
    x, y = U.onehot(fx["codes"]).cuda(), torch.from_numpy(fx["y"]).cuda()
    sym = torch.empty((x.shape[0], x.shape[2]), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().mural_op_dense_to_symbols(x.data_ptr(), x.shape[0], x.shape[2], sym.data_ptr(), status.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    res = []
    for inp in (x, SymbolWindows(sym)):
        m = product_from(fx)
        m.load_state_dict(U.indel_state_for(fx, orc), strict=True)
        m = m.cuda().train()
        m.out_fc[1].p = 0.0
        preds, loss = _train_step(m, inp, y)
        res.append((preds.detach(), loss.item(), [p.grad.clone() for p in m.parameters()]))
    (p0, l0, g0), (p1, l1, g1) = res
    assert float((p0 - p1).abs().max()) <= 1e-5 * max(1.0, float(p0.abs().max())) and abs(l0 - l1) <= 1e-5 * abs(l0)
    for a, b in zip(g0, g1):
        assert torch.isfinite(b).all() and float((a - b).abs().max()) <= 2e-4 * (float(a.abs().max()) + 1e-2)
    print("PRODUCT_INDEL_SYMBOLS_OK")


if __name__ == "__main__":
    main()
