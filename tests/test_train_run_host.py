"""Host logic of a training run (mural_amd.train_run, tools/train_files.py): early stopping on hand-written loss sequences, the text of
the per-epoch metrics file, the --weight_decay_auto arithmetic, the refusal of the reference's unsupported flags, the checkpoint file
names.  No GPU."""
import importlib.util
import os
import pickle

import pytest
import torch

from mural_amd import train_run as R


def _tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_files.py")
    spec = importlib.util.spec_from_file_location("train_files_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(losses, patience):
    """(epoch the run ends at, counter, best epoch by the reference's arithmetic, log) of the loop's use of the stopper."""
    log = []
    stopper = R.EarlyStopping(patience=patience, verbose=True, trace_func=log.append)
    epoch = -1
    for epoch, loss in enumerate(losses):
        stopper(loss, None)
        if stopper.early_stop:
            break
    return epoch, stopper.counter, epoch - stopper.counter, log


def test_early_stopping_on_hand_written_sequences():
    # improving all the way: never stops, the last epoch is the best
    assert _run([5.0, 4.0, 3.0, 2.0], 2)[:3] == (3, 0, 3)
    # best at epoch 1, then two epochs without improvement trip patience 2 at epoch 3
    end, counter, best, log = _run([5.0, 4.0, 4.5, 4.2, 1.0, 0.5], 2)
    assert (end, counter, best) == (3, 2, 1)
    assert log[-2:] == ["EarlyStopping counter: 1 out of 2", "EarlyStopping counter: 2 out of 2"]
    assert log[0] == "Validation loss decreased (inf --> 5.000000)."
    # an improvement resets the counter: 1 bad, better, 2 bad
    assert _run([3.0, 3.5, 2.0, 2.1, 2.2, 0.1], 2)[:3] == (4, 2, 2)
    # an equal loss counts as an improvement (score < best is false), as in the reference: a constant loss never stops a run
    assert _run([2.0] * 6, 1)[:3] == (5, 0, 5)
    # patience 1: the first worse epoch ends the run
    assert _run([2.0, 2.5, 1.0], 1)[:3] == (1, 1, 0)
    s = R.EarlyStopping(patience=3)
    assert (s.counter, s.early_stop, s.best_score) == (0, False, None)
    s(1.0, object())
    assert s.best_score == -1.0 and s.val_loss_min == 1.0
    # delta: an improvement smaller than delta does not count
    d = R.EarlyStopping(patience=5, delta=0.1, trace_func=lambda *_: None)
    d(1.0)
    d(0.95)
    assert d.counter == 1
    d(0.85)
    assert d.counter == 0 and d.best_score == -0.85


def test_metrics_text_and_file(tmp_path):
    m = dict(score=17.25, total_params=12345, loss=0.25, after_min_loss=2, fdiri_loss=0.2498, extra="not written")
    want = "loss: 0.25\nfdiri_loss: 0.2498\nafter_min_loss: 2\nscore: 17.25\ntotal_params: 12345\n"
    assert R.metrics_text(m) == want
    assert R.METRIC_KEYS == ("loss", "fdiri_loss", "after_min_loss", "score", "total_params")
    model = R.checkpoint_path(tmp_path, 3)
    assert model == os.path.join(str(tmp_path), "checkpoint_3", "model") and os.path.isdir(os.path.dirname(model))
    path = R.write_metrics(m, tmp_path, 3)
    assert path == os.path.join(str(tmp_path), "checkpoint_3", "epoch_3_metrics.txt") and open(path).read() == want
    # floats are written by repr, as an f-string does
    assert R.metrics_text(dict(m, loss=1 / 3)).splitlines()[0] == f"loss: {1 / 3}"
    with pytest.raises(KeyError):
        R.metrics_text({"loss": 1.0})


def test_checkpoint_file_names(tmp_path):
    """save_model into checkpoint_path: the three files of a reference checkpoint, loadable without a device."""
    import numpy as np
    from mural_amd.calibration import load_dirichlet_weights
    from mural_amd.model.nn_utils import load_model_config, save_model
    net = torch.nn.Linear(3, 2)
    w = np.hstack([np.eye(4), np.zeros((4, 1))]) + 0.125
    cfg = dict(model_no=2, n_class=4, emb_dims=[(65, 2)] * 3, down_list=[1, 2], learning_rate=1e-3)
    for epoch in (0, 11):
        path = R.checkpoint_path(tmp_path / "trial", epoch)
        save_model(net, w, cfg, path)
        R.write_metrics(dict(loss=1.0, fdiri_loss=1.0, after_min_loss=0, score=2.0, total_params=8), tmp_path / "trial", epoch)
        assert sorted(os.listdir(tmp_path / "trial" / f"checkpoint_{epoch}")) == [f"epoch_{epoch}_metrics.txt", "model", "model.config.pkl",
                                                                               "model.fdiri_cal.pkl"]
        assert load_model_config(path + ".config.pkl") == cfg
        assert np.array_equal(load_dirichlet_weights(path + ".fdiri_cal.pkl"), w)
        state = torch.load(path, map_location="cpu", weights_only=True)
        assert sorted(state) == ["bias", "weight"] and torch.equal(state["weight"], net.weight.detach())
    with open(path + ".config.pkl", "rb") as f:
        assert pickle.load(f) == cfg


def test_weight_decay_auto_arithmetic():
    # training.py:343: 1 - auto ** (batch_size / (epochs * train_size))
    assert R.auto_weight_decay(0.1, 128, 10, 1_000_000) == 1 - 0.1 ** (128 / (10 * 1_000_000))
    got = R.auto_weight_decay(0.5, 64, 2, 6400)
    assert got == 1 - 0.5 ** (64 / 12800)
    # the decay per step, applied over the run's steps, leaves `auto` of a weight
    steps = 2 * 6400 / 64
    assert abs((1 - got) ** steps - 0.5) < 1e-12
    for bad in (1.0, 1.5, 0.0, -0.1):
        with pytest.raises(ValueError, match="smaller than 1"):
            R.auto_weight_decay(bad, 64, 2, 6400)


def test_default_emb_dims():
    assert R.default_emb_dims(7, 3) == [(65, 2)] * 13              # 4 ** 3 k-mers + the padding id; int(65 ** 0.25) == 2
    assert R.default_emb_dims(5, 2) == [(17, 2)] * 10
    assert R.default_emb_dims(2, 1) == [(5, 1)] * 5
    assert R.default_emb_dims(5, 2, "indel") == [(17, 2)] * 9       # an INDEL local window has no middle column


@pytest.mark.parametrize("flags", [["--bw_paths", "tracks.txt"], ["--with_h5"], ["--use_ray", "--n_trials", "4"], ["--h5f_path=x.h5"],
                                   ["--sample_weights", "w.txt"]])
def test_unsupported_reference_flags_are_refused_in_one_line(flags, capsys):
    tool = _tool()
    argv = ["--ref_genome", "g.fa", "--train_data", "s.bed"] + flags
    with pytest.raises(SystemExit) as e:
        tool.main(argv)
    msg = str(e.value.code)
    assert "\n" not in msg and "not supported" in msg and "DESIGN.md section 6" in msg
    for f in flags:
        if f.startswith("--"):
            assert f.partition("=")[0] in msg
    assert capsys.readouterr().out == ""                          # refused before anything is read or printed


def test_tool_takes_the_reference_flag_names():
    tool = _tool()
    argv = ("--ref_genome g.fa --train_data s.bed --validation_data v.bed --valid_ratio 0.2 --split_seed 7 --model_no 2 --n_class 4 "
            "--local_radius 5 --local_order 2 --local_hidden1_size 64 --local_hidden2_size 0 --distal_radius 110 --emb_dropout 0.1 "
            "--local_dropout 0.2 --distal_fc_dropout 0.3 --CNN_kernel_size 3 --CNN_out_channels 32 --segment_center 2000 "
            "--sampled_segments 2 --batch_size 64 --optim AdamW --learning_rate 0.002 --lr_scheduler ROP --weight_decay 1e-4 "
            "--weight_decay_auto 0.2 --restart_lr 1e-4 --min_lr 1e-6 --LR_gamma 0.5 --epochs 3 --grace_period 2 --poisson_calib "
            "--save_valid_preds --experiment_name run1 --model_type snv --model_path m --model_config_path m.config.pkl "
            "--init_fc_with_pretrained").split()
    tool.reject_unsupported(argv)
    args = tool.parser().parse_args(argv)
    cfg = tool.build_config(args)
    assert cfg["local_hidden2_size"] == 32 and cfg["lr_scheduler"] == "ROP" and cfg["optim"] == "AdamW" and cfg["batch_size"] == 64
    assert cfg["n_class"] == 4 and cfg["model_no"] == 2 and cfg["distal_radius"] == 110 and cfg["seq_only"] is True
    assert cfg["transfer_learning"] is True and args.init_fc_with_pretrained and args.poisson_calib and args.save_valid_preds
    indel = tool.parser().parse_args("--ref_genome g.fa --train_data s.bed --model_type indel --down_list 1 2 5 1 1 2 --use_reverse".split())
    cfg = tool.build_config(indel)
    assert cfg["down_list"] == [1, 2, 5, 1, 1, 2] and cfg["use_reverse"] is True and cfg["n_class"] == 8 and cfg["model_no"] == 0
    assert cfg["distal_radius"] == 4000 and "local_hidden1_size" not in cfg
