"""Train a model from a FASTA + BED pair and write a reference-style trial directory (what `mural_snv train` / `mural_indel train` /
`transfer` do without Ray): python tools/train_files.py --ref_genome FASTA --train_data BED [options]

The options carry the reference's names (MuRaL/commands/train.py, transfer.py); one value each, no hyper-parameter search:
  data       --ref_genome --train_data --validation_data --valid_ratio (0.1) --split_seed (random when negative)
  model      --model_type snv|indel  --model_no --n_class --local_radius --local_order --local_hidden1_size --local_hidden2_size
             --distal_radius --emb_dropout --local_dropout --distal_fc_dropout --CNN_kernel_size --CNN_out_channels
             INDEL: --down_list N N N N N N  --use_reverse
  batches    --segment_center --sampled_segments --batch_size
  optimiser  --optim Adam|AdamW|AdamW2|SGD --learning_rate --lr_scheduler StepLR|StepLR2|ROP --weight_decay --weight_decay_auto
             --restart_lr --min_lr --LR_gamma
  run        --epochs --grace_period --poisson_calib --save_valid_preds --experiment_name  [--trial_dir DIR] [--host_loop]
  transfer   --model_path --model_config_path --init_fc_with_pretrained

Output: <trial_dir>/checkpoint_<epoch>/{model, model.config.pkl, model.fdiri_cal.pkl, epoch_<epoch>_metrics.txt}; the trial directory
defaults to results/<experiment_name>/trial.  A checkpoint is what tools/predict_files.py takes as MODEL.  bigWig tracks, HDF5 caches, Ray
and sample weights are out of scope: their flags are refused."""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

UNSUPPORTED = ("--bw_paths", "--without_bw_distal", "--with_h5", "--h5f_path", "--n_h5_files", "--use_ray", "--n_trials", "--ASHA_metric",
               "--ray_ncpus", "--ray_ngpus", "--cpu_per_trial", "--gpu_per_trial", "--rerun_failed", "--sample_weights", "--ImbSampler",
               "--custom_dataloader")


def reject_unsupported(argv):
    """SystemExit with one line that names the reference flags in `argv` this tool does not take."""
    bad = sorted({a.partition("=")[0] for a in argv if a.partition("=")[0] in UNSUPPORTED})
    if bad:
        raise SystemExit(f"train_files: {', '.join(bad)}: not supported -- bigWig tracks, HDF5 caches, Ray tuning and sample weights are "
                         "out of scope (DESIGN.md section 6); sequence-only models, one trial")


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    a = ap.add_argument
    a("--ref_genome", required=True)
    a("--train_data", required=True)
    a("--validation_data", default=None)
    a("--valid_ratio", type=float, default=0.1)
    a("--split_seed", type=int, default=-1)
    a("--distal_order", type=int, default=1, choices=[1], help="accepted: the distal windows are order-1 one-hot")
    a("--seq_only", action="store_true", help="accepted: every model here is sequence-only")
    a("--model_type", default="snv", choices=["snv", "indel"])
    a("--model_no", type=int, default=None, help="default 2 (snv) / 0 (indel)")
    a("--n_class", type=int, default=None, help="default 4 (snv) / 8 (indel)")
    a("--local_radius", type=int, default=7)
    a("--local_order", type=int, default=3)
    a("--local_hidden1_size", type=int, default=150)
    a("--local_hidden2_size", type=int, default=0, help="0: half of --local_hidden1_size")
    a("--distal_radius", type=int, default=None, help="default 200 (snv) / 4000 (indel)")
    a("--emb_dropout", type=float, default=0.1)
    a("--local_dropout", type=float, default=0.1)
    a("--distal_fc_dropout", type=float, default=0.25)
    a("--CNN_kernel_size", type=int, default=3)
    a("--CNN_out_channels", type=int, default=32)
    a("--down_list", type=int, nargs="+", default=[1, 2, 5, 5, 5, 8])
    a("--use_reverse", action="store_true")
    a("--segment_center", type=int, default=300000)
    a("--sampled_segments", type=int, default=10)
    a("--batch_size", type=int, default=128)
    a("--optim", default="Adam", choices=["Adam", "AdamW", "AdamW2", "SGD"])
    a("--learning_rate", type=float, default=0.001)
    a("--lr_scheduler", default="StepLR", choices=["StepLR", "StepLR2", "ROP"])
    a("--weight_decay", type=float, default=1e-5)
    a("--weight_decay_auto", type=float, default=0.1)
    a("--restart_lr", type=float, default=1e-4)
    a("--min_lr", type=float, default=1e-6)
    a("--LR_gamma", type=float, default=0.9)
    a("--epochs", type=int, default=10)
    a("--grace_period", type=int, default=5)
    a("--poisson_calib", action="store_true")
    a("--save_valid_preds", action="store_true")
    a("--experiment_name", default=None, help="default snv_experiment / indel_experiment")
    a("--trial_dir", default=None, help="default results/<experiment_name>/trial")
    a("--host_loop", action="store_true", help="train_epoch (host scheduler) instead of the device loop")
    a("--cuda_id", default="0")
    a("--model_path", default=None)
    a("--model_config_path", default=None)
    a("--train_all", action="store_true", help="accepted: transfer learning here always trains every parameter")
    a("--init_fc_with_pretrained", action="store_true")
    return ap


def build_config(args):
    """The reference's config dict of one trial (run_train_raytune.py:200-230) from the parsed options."""
    indel = args.model_type == "indel"
    cfg = dict(local_radius=args.local_radius, local_order=args.local_order, distal_radius=args.distal_radius or (4000 if indel else 200),
               CNN_kernel_size=args.CNN_kernel_size, CNN_out_channels=args.CNN_out_channels, segment_center=args.segment_center,
               sampled_segments=args.sampled_segments, batch_size=args.batch_size, optim=args.optim, learning_rate=args.learning_rate,
               lr_scheduler=args.lr_scheduler, weight_decay=args.weight_decay, LR_gamma=args.LR_gamma, restart_lr=args.restart_lr,
               min_lr=args.min_lr, n_class=args.n_class or (8 if indel else 4), model_no=args.model_no if args.model_no is not None else
               (0 if indel else 2), seq_only=True, without_bw_distal=False, transfer_learning=args.model_path is not None)
    if indel:
        cfg.update(down_list=list(args.down_list), use_reverse=bool(args.use_reverse))
    else:
        cfg.update(local_hidden1_size=args.local_hidden1_size, emb_dropout=args.emb_dropout, local_dropout=args.local_dropout,
                   local_hidden2_size=args.local_hidden2_size if args.local_hidden2_size > 0 else args.local_hidden1_size // 2,
                   distal_fc_dropout=args.distal_fc_dropout)
    return cfg


def main(argv):
    reject_unsupported(argv)
    args = parser().parse_args(argv)
    if (args.model_path is None) != (args.model_config_path is None):
        raise SystemExit("train_files: transfer learning takes --model_path and --model_config_path together")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_files: no HIP device (mural_amd has no CPU path)")
    from mural_amd import train_run as R
    from mural_amd.data import EpochLoader
    from mural_amd.model.nn_utils import load_model_config
    device = torch.device("cuda", int(args.cuda_id))
    torch.cuda.set_device(device)
    cfg = build_config(args)
    if args.model_path is not None:      # the pretrained model's architecture; this run's batches, optimiser and schedule (transfer.py)
        old = load_model_config(args.model_config_path)
        keep = ("segment_center", "sampled_segments", "batch_size", "optim", "learning_rate", "lr_scheduler", "weight_decay", "LR_gamma",
                "restart_lr", "min_lr", "transfer_learning")
        cfg = {**old, **{k: cfg[k] for k in keep}, "init_fc_with_pretrained": bool(args.init_fc_with_pretrained), "train_all": True}
    indel = args.model_type == "indel"
    if args.split_seed < 0:
        args.split_seed = random.randint(0, 1000000)
    print("args.split_seed:", args.split_seed)
    kw = dict(segment_center=cfg["segment_center"], sampled_segments=cfg["sampled_segments"], model_type=args.model_type, device=device,
              symbols=indel)
    loader = EpochLoader(args.ref_genome, args.train_data, cfg["batch_size"], cfg["local_radius"], cfg["local_order"], cfg["distal_radius"], **kw)
    if args.validation_data:
        print("using given validation file:", args.validation_data)
        train = loader
        valid = EpochLoader(args.ref_genome, args.validation_data, cfg["batch_size"], cfg["local_radius"], cfg["local_order"],
                            cfg["distal_radius"], genomes=loader.genomes, **kw)
    else:
        train, valid = loader.split(args.valid_ratio, args.split_seed)
    if args.weight_decay_auto is not None and args.weight_decay_auto > 0:
        try:
            cfg["weight_decay"] = R.auto_weight_decay(args.weight_decay_auto, cfg["batch_size"], args.epochs, len(train))
        except ValueError as e:
            raise SystemExit(str(e)) from None
        print("NOTE: rewriting config['weight_decay'], new weight_decay: ", cfg["weight_decay"])
    try:
        model = R.prepare_model(cfg, device, model_path=args.model_path, init_fc_with_pretrained=args.init_fc_with_pretrained or
                                args.model_path is None, model_type=args.model_type)
    except ValueError as e:
        raise SystemExit(f"train_files: {e}") from None
    name = args.experiment_name or f"{args.model_type}_experiment"
    trial_dir = args.trial_dir or os.path.join("results", name, "trial")
    os.makedirs(trial_dir, exist_ok=True)
    history, best = R.fit(model, cfg, train, valid, epochs=args.epochs, trial_dir=trial_dir, grace_period=args.grace_period, device=device,
                          model_type=args.model_type, device_loop=not args.host_loop, split_generator_seed=args.split_seed,
                          save_valid_preds=args.save_valid_preds, poisson_calib=args.poisson_calib)
    print(f"{len(history)} epochs -> {trial_dir}; best checkpoint: {os.path.join(trial_dir, f'checkpoint_{best}', 'model')}")


if __name__ == "__main__":
    main(sys.argv[1:])
