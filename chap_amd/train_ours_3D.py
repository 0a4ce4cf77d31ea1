"""train(args, snapshot_path) for the 3D configuration (LA, V-Net DualDecoder3d, 112 x 112 x 80 patches): the host loop of
chap_amd/train_ours_2D.py around the same captured iteration (ChapStep, dims 3).  Upstream has no 3D training script (SURVEY
section 1.5): the loop, its outputs (`latest.pth`, `{model}_best_model.pth`, `val.csv`, `log.txt`) and its flags are those of
code/train_ours_2D.py:219-463; the data layer and the validation are this project's definition (DESIGN.md "3D workflow", unpinned).

Data, the first that is present: `args["trainloader"]` (any iterable of {'image': [B,1,P0,P1,P2] fp32, 'label': [B,P0,P1,P2]} dicts; a
loader with `next_into`, chap_amd.data.DeviceLoader, feeds the captured iteration through ChapStep.stage_from); `args["root_path"]` +
`args["labeled_num"]` (the LA h5 layout of test_LA.py:25-28: the first `labeled_num` cases of `train.list` are the labelled ones,
volumes resident on the device, random crops zero-padded where a volume is smaller than the patch); else the fixed-seed synthetic
generator.  Validation: `args["val_volumes"]`, a list of (image [w,h,d], label [w,h,d]) arrays, scored by the sliding window of
chap_amd.test_3d_patch.var_all_case (mean foreground Dice, first decoder: binary, whatever `num_classes` (2..8) is -- per-class 3D
validation is not built).  `dropout=True` is unsupported in 3D (ChapStep raises).
`args["has_residual"]` (default False) builds the network with residual V-Net blocks (vnet.py:37-67).

`args["data_parallel"]`: this process is one rank of the run, exactly as in chap_amd/train_ours_2D.py (see there and DESIGN.md section 6
"train() on several ranks"): per-rank `batch_size` / `labeled_bs`, the rank's shard of the DeviceLoader built here, the fold-schedule gradient
exchange, validation split over the ranks case by case (var_each_case below, the mean taken over the gathered values in case order),
files written by rank 0 alone.  The loss line of every 50th iteration is rank 0's LOCAL values."""
import csv
import logging
import os
import time

import numpy as np
import torch

from .distributed import attach_step, flush_monitor, init_rank, sync_for_validation
from .guard import StepGuard, check_finite_before_save, flush_to_run as flush_guard
from .monitor import StepMonitor
from .networks.net_factory_3d import net_factory_3d
from .networks.vnet import DualDecoder3d, VNet
from .synthetic import synthetic_batch_3d
from . import metrics
from . import test_3d_patch as T3P
from .train import DEFAULT_ARGS, ChapStep, build_teacher, check_num_classes, check_optimizer, check_teacher_consistency, check_teacher_uncertainty, optimizer_line, uncertainty_threshold

FLAG_DEFAULTS = dict(DEFAULT_ARGS, model="dualdecoder", num_classes=2, patch_size=[112, 112, 80], batch_size=4, labeled_bs=2,
                     stride_xy=18, stride_z=4, val_interval=200, use_graph=True, gpu=0, seed=1337,
                     mean_teacher=False, ema_decay=0.99, monitor=False,       # as train_ours_2D: --ema_decay (train_ours_2D.py:499), the ema_model of :251
                     clip_grad_norm=0.0, skip_nonfinite=False,                # chap_amd.guard, as train_ours_2D
                     optimizer="sgd", betas=(0.9, 0.999), adam_eps=1e-8,               # chap_amd.train.FusedAdamW: 'adam' (L2 weight decay) / 'adamw' (decoupled) with base_lr, weight_decay
                     data_parallel=False, dp_backend="nccl", dp_timeout_s=600, dp_force_group=False, dp_noise_per_rank=True)      # chap_amd.distributed


def _synthetic_loader(a, rank=0):
    lbs, ubs = a["labeled_bs"], a["batch_size"] - a["labeled_bs"]
    pool = [synthetic_batch_3d(a["seed"] + 4 * rank + i, lbs, ubs, *a["patch_size"], n_classes=a["num_classes"]) for i in range(4)]      # a pool of its own per data-parallel rank
    while True:
        for v, l in pool:
            yield {"image": v, "label": l}


def var_each_case(model, image_list, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4):
    """test_3d_patch.var_all_case's per-case foreground Dice values as a list, in the order of `image_list` (which may be empty): the same
    window, the same counts-only metrics launch per case.  A data-parallel rank scores its shard of the cases with it; the mean is then taken
    over the gathered values in case order, with var_all_case's arithmetic (0.0 + d0 + d1 + ..., divided by the count)."""
    device = T3P._model_device(model)
    out = []
    for entry in image_list:
        image, label = T3P._load_case(entry)
        pred, _ = T3P._predict_device(model, image, stride_xy, stride_z, patch_size, num_classes, T3P.WINDOW_BATCH, device, average=False)
        with torch.cuda.device(device):
            out.append(metrics.dc(pred.contiguous(), label))
    return out


def train(args, snapshot_path):
    a = dict(FLAG_DEFAULTS)
    a.update(args)
    check_num_classes(a["num_classes"], "chap_amd.train_ours_3D")
    check_optimizer(a["optimizer"], "chap_amd.train_ours_3D")
    check_teacher_consistency(a, bool(a["mean_teacher"]), "chap_amd.train_ours_3D")        # before a directory or a file is made
    check_teacher_uncertainty(a, "chap_amd.train_ours_3D")
    ctx = init_rank(a)                          # the plain single process unless args["data_parallel"]
    log = logging.getLogger("chap_amd.train3d")
    log.setLevel(logging.INFO)
    fh = None
    try:
        if ctx.is_main:                         # rank 0 alone writes under snapshot_path
            os.makedirs(snapshot_path, exist_ok=True)
            fh = logging.FileHandler(os.path.join(snapshot_path, "log.txt"))
            log.addHandler(fh)
        if a["optimizer"] != "sgd":              # (the default run's log is what it always was)
            log.info(optimizer_line(a))
        device = ctx.device
        if ctx.group is not None:
            torch.cuda.set_device(device)
        torch.manual_seed(a["seed"])
        np.random.seed(a["seed"])               # on every rank: ONE BCP box per iteration for the global batch
        def make():
            if a.get("has_residual", False):
                # ResidualConvBlock nets (vnet.py:37-67): net_factory_3d keeps the reference's signature, which has no such flag, so the class is built
                # here with the factory's train-mode arguments
                cls = {"vnet": VNet, "dualdecoder": DualDecoder3d}.get(a["model"])
                kw = dict(args=a) if cls is DualDecoder3d else {}
                return cls(n_channels=1, n_classes=a["num_classes"], normalization="batchnorm", has_dropout=True, has_residual=True, **kw).to(device) if cls else None
            return net_factory_3d(net_type=a["model"], in_chns=1, class_num=a["num_classes"], mode="train", device=device, args=a)

        model = make()
        if model is None:
            raise ValueError("chap_amd.train_ours_3D: no 3D network named %r" % (a["model"],))
        model.train()
        if a.get("dtype", "fp32") == "bf16":
            model.set_compute_dtype(torch.bfloat16)
        # monitor: per-iteration pseudo-label quality from inside the step (chap_amd.monitor), read every val_interval iterations
        mon = StepMonitor(a["num_classes"], ring=max(256, int(a["val_interval"])), device=device) if a["monitor"] else None
        step_kw = {} if mon is None else {"monitor": mon}
        # guard: clip by the global gradient norm and / or skip non-finite steps inside the optimizer launch (chap_amd.guard), read like the monitor
        guard = None
        if float(a["clip_grad_norm"]) > 0 or a["skip_nonfinite"]:
            guard = StepGuard(max_norm=float(a["clip_grad_norm"]), skip_nonfinite=bool(a["skip_nonfinite"]), ring=max(256, int(a["val_interval"])), device=device)
            step_kw["guard"] = guard
        if ctx.group is not None:                   # one replica of several: the fused SGD scales the summed gradient by 1 / world
            step_kw["world_size"] = ctx.world
        if a["mean_teacher"]:                   # ema_model = create_model(ema=True) (train_ours_2D.py:238-251)
            teacher = build_teacher(make).eval()
            step = ChapStep(model, a, teacher=teacher, **step_kw)
        else:
            teacher, step = None, ChapStep(model, a, **step_kw)
        attach_step(ctx, step, a)               # (data-parallel) rank 0's weights everywhere, the gradient exchange, the rank's noise stream
        loader = a.get("trainloader")
        if loader is None and a.get("root_path") and a.get("labeled_num"):
            from .data import DeviceLoader, VolumeStore
            store = VolumeStore.from_h5_list(a["root_path"], device=device)
            n_lab = int(a["labeled_num"])
            loader = DeviceLoader(store, range(n_lab), range(n_lab, len(store)), a["batch_size"], a["labeled_bs"], a["patch_size"], a["seed"], pad=True,
                                  rank=ctx.rank, world=ctx.world)
        loader = loader or _synthetic_loader(a, ctx.rank)
        device_fed = a["use_graph"] and hasattr(loader, "next_into")      # the next batch is built on the device, beside the running iteration
        val = a.get("val_volumes")
        if val is None:
            vi, vl = synthetic_batch_3d(a["seed"] + 4242, 1, 0, *a["patch_size"], n_classes=a["num_classes"])
            val = [(vi[0, 0].numpy(), vl[0].numpy())]
        best, ema_best, captured = 0.0, -1.0, False         # (the first validated teacher is the best so far, whatever it scores)

        def validate(net):
            # each rank scores its shard of the cases; the sum runs over the gathered values in case order: var_all_case's arithmetic
            per = var_each_case(net, ctx.shard(val), a["num_classes"], tuple(a["patch_size"]), a["stride_xy"], a["stride_z"])
            total = 0.0
            for d in ctx.gather_in_order(per, len(val)):
                total += d
            return float(total / len(val))

        def batches():
            """train_ours_2D.py:299-302, 459-463: a finite loader is re-iterated until max_iterations is reached; one that yields nothing ends
            the run, loudly."""
            while True:
                n = 0
                for b in loader:
                    n += 1
                    yield b
                if n == 0:
                    raise RuntimeError("chap_amd.train_ours_3D: the train loader yielded no batch (exhausted one-shot iterator or empty dataset) "
                                       "at iteration %d of %d" % (step.iter_num, a["max_iterations"]))

        gen = batches()
        sampled_batch = next(gen)
        while True:
            if a["use_graph"]:
                if not captured:
                    step.capture(sampled_batch["image"].to(device), sampled_batch["label"].to(device))
                    captured = True
                    step.stage(sampled_batch["image"], sampled_batch["label"])
                out = step.replay()
            else:
                out = step.step(sampled_batch["image"].to(device, non_blocking=True), sampled_batch["label"].to(device, non_blocking=True))
            it = step.iter_num
            if it % 50 == 0:
                log.info("iteration %d : bcp loss : %f vat loss : %f" % (it, sum(float(l[2]) for l in out["mix_losses"]), float(out["vat_loss"])))
            if "teacher_loss" in out and (it % 50 == 0 or it >= a["max_iterations"]):      # only with teacher_consistency > 0 (the default run's log is what it always was); the last iteration closes the record
                if "teacher_certain" in out:       # teacher_uncertainty > 0: the share of pixels the term counted, and the entropy threshold of this iteration
                    log.info("iteration %d : teacher loss : %f : certain share : %f : entropy threshold : %f" % (
                        it, float(out["teacher_loss"]), float(out["teacher_certain"]) / step.teacher_pixels, uncertainty_threshold(it - 1, a)))
                else:
                    log.info("iteration %d : teacher loss : %f" % (it, float(out["teacher_loss"])))
            if it > 0 and it % a["val_interval"] == 0:
                sync_for_validation(ctx, step)   # (data-parallel) replicas equal, else raise; rank 0's BatchNorm statistics into every replica
                model.eval()
                dice = validate(model)
                # the checkpoint gate, on every rank (the replicas are equal: the same decision everywhere): no file is overwritten with a non-finite model
                check_finite_before_save(model.state_dict(), "the model", it)
                if ctx.is_main:
                    torch.save(model.state_dict(), os.path.join(snapshot_path, "latest.pth"))
                if dice > best:                 # the same decision on every rank: `dice` is the same word everywhere
                    best = dice
                    if ctx.is_main:
                        torch.save(model.state_dict(), os.path.join(snapshot_path, "{}_best_model.pth".format(a["model"])))
                        with open(os.path.join(snapshot_path, "val.csv"), "a", newline="") as f:
                            csv.writer(f).writerow([time.strftime("%Y-%m-%d %H:%M:%S"), it, round(best, 4)])
                log.info("iteration %d : dice_score : %f" % (it, dice))
                if teacher is not None:         # the averaged weights with the student's current BatchNorm statistics, after the student, same function
                    step.sync_teacher_stats()
                    ema_dice = validate(teacher)
                    check_finite_before_save(teacher.state_dict(), "the mean teacher", it)
                    if ctx.is_main:
                        torch.save(teacher.state_dict(), os.path.join(snapshot_path, "ema_latest.pth"))
                    if ema_dice > ema_best:
                        ema_best = ema_dice
                        if ctx.is_main:
                            torch.save(teacher.state_dict(), os.path.join(snapshot_path, "{}_ema_best_model.pth".format(a["model"])))
                    log.info("iteration %d : ema_dice_score : %f" % (it, ema_dice))
                model.train()
                ctx.barrier()                   # no rank runs ahead of a half-written checkpoint
            if mon is not None and (it % a["val_interval"] == 0 or it >= a["max_iterations"]):
                flush_monitor(ctx, mon, snapshot_path, log)
            if guard is not None and ctx.is_main and (it % a["val_interval"] == 0 or it >= a["max_iterations"]):
                flush_guard(guard, snapshot_path, log)       # rank 0 alone: the rows are the same words on every rank
            if it >= a["max_iterations"]:
                break
            if device_fed:
                step.stage_from(loader)
                continue
            sampled_batch = next(gen)
            if a["use_graph"]:
                step.stage(sampled_batch["image"], sampled_batch["label"])      # travels while the iteration enqueued above runs
        ctx.barrier()
    finally:                    # also when the loop raises: leave the process groups; a later train() in this process must not log into this file
        ctx.close()
        if fh is not None:
            log.removeHandler(fh)
            fh.close()
    return model
