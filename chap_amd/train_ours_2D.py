"""train(args, snapshot_path): the thin host loop around the MI355X iteration, with the reference's entry-point
signature and outputs (code/train_ours_2D.py:219-463): `args` is the dict of its argparse flags (`vars(args)`, :525-526);
it writes `latest.pth` and `{model}_best_model.pth` (= torch.save(model.state_dict()), :428-435), `val.csv` (:437-449)
and `log.txt` (:567-570) under `snapshot_path`.  `args["monitor"]` (default off; chap_amd.monitor) adds `monitor.csv`, one line per
iteration, and the reference's per-iteration `l loss` / `unl loss` line (:404-405) to `log.txt`, both written once per validation interval.

What is NOT here (out of scope): TensorBoard / wandb, the validation-set reader.  The data layer is an
argument: `args["trainloader"]` / `args["val_volumes"]` may carry any iterable of {'image': [B,1,H,W] fp32, 'label': [B,H,W]}
dicts / list of (image [1,S,H,W], label [1,S,H,W]) tensors (what the reference's valloader yields, :274).  A loader with
`next_into` (chap_amd.data.DeviceLoader: slices resident on the device, RandomGenerator as one kernel per batch) feeds the
captured iteration through ChapStep.stage_from; `args["root_path"]` + `args["labeled_slices"]` (the number of labelled slices at
the head of `train_slices.list`; the reference's patient -> slice table is not copied) build that loader from the ACDC h5 layout.
With none of them the fixed-seed synthetic generator of chap_amd.synthetic stands in.

`args["data_parallel"]` (default off; chap_amd.distributed, DESIGN.md section 6 "train() on several ranks"): this process is ONE RANK of the
run, started by `python -m chap_amd.launch` or `torch.distributed.run`.  `batch_size` / `labeled_bs` are per rank; the DeviceLoader built
here is the rank's shard of the global batch (a loader passed in `trainloader` is taken as already being the rank's own); gradients go
through the fold schedule of chap_amd.parallel; at a validation interval the replicas are checked for equality, rank 0's BatchNorm statistics
are broadcast, every rank scores val_volumes[rank::world] and the mean is taken over the gathered per-volume values in volume order, so every
rank takes the same "best" decision; rank 0 alone writes files (a barrier follows).  The loss line of every 50th iteration stays rank 0's
LOCAL values (its own shard); the monitor's rows are merged over the ranks (monitor.merge_rows).  `dp_backend` ("nccl" | "gloo": all
ranks on cuda:`gpu`, the one-GPU rehearsal), `dp_timeout_s`, `dp_force_group` (a 1-rank group), `dp_noise_per_rank` (default True)."""
import csv
import logging
import os
import time

import numpy as np
import torch

from .distributed import attach_step, flush_monitor, init_rank, sync_for_validation
from .inference import test_single_volume
from .guard import StepGuard, check_finite_before_save, flush_to_run as flush_guard
from .monitor import StepMonitor
from .networks.net_factory import net_factory
from .synthetic import synthetic_batch
from .train import DEFAULT_ARGS, ChapStep, build_teacher, check_num_classes, check_optimizer, check_teacher_consistency, check_teacher_uncertainty, optimizer_line, uncertainty_threshold

FLAG_DEFAULTS = dict(DEFAULT_ARGS, model="dualdecoder", decoder_type="mcnet", gpu=0, seed=1337, image_size=[256, 256],
                     val_interval=200, labeled_num=7, use_graph=True,          # train_ours_2D.py:469-526
                     mean_teacher=False, ema_decay=0.99,                       # --ema_decay (:499); mean_teacher: the commented-out ema_model (:251)
                     monitor=False,                                            # chap_amd.monitor: monitor.csv and the loss line of :404-405
                     clip_grad_norm=0.0, skip_nonfinite=False,                 # chap_amd.guard: clip by the global gradient norm (0 = off), skip non-finite steps; guard.csv
                     optimizer="sgd", betas=(0.9, 0.999), adam_eps=1e-8,               # chap_amd.train.FusedAdamW: 'adam' (L2 weight decay) / 'adamw' (decoupled) with base_lr, weight_decay
                     data_parallel=False, dp_backend="nccl", dp_timeout_s=600, dp_force_group=False, dp_noise_per_rank=True)      # chap_amd.distributed


def _synthetic_loader(a, rank=0):
    h, w = a["image_size"]
    lbs, ubs = a["labeled_bs"], a["batch_size"] - a["labeled_bs"]
    pool = [synthetic_batch(a["seed"] + 8 * rank + i, lbs, ubs, h, w, a["num_classes"]) for i in range(8)]      # a pool of its own per data-parallel rank
    while True:
        for v, l in pool:
            yield {"image": v, "label": l}


def train(args, snapshot_path):
    a = dict(FLAG_DEFAULTS)
    a.update(args)
    check_num_classes(a["num_classes"], "chap_amd.train_ours_2D")
    check_optimizer(a["optimizer"], "chap_amd.train_ours_2D")
    check_teacher_consistency(a, bool(a["mean_teacher"]), "chap_amd.train_ours_2D")        # before a directory or a file is made
    check_teacher_uncertainty(a, "chap_amd.train_ours_2D")
    ctx = init_rank(a)                          # the plain single process unless args["data_parallel"]
    log = logging.getLogger("chap_amd.train")
    log.setLevel(logging.INFO)
    fh = None
    try:
        if ctx.is_main:                         # rank 0 alone writes under snapshot_path
            os.makedirs(snapshot_path, exist_ok=True)
            fh = logging.FileHandler(os.path.join(snapshot_path, "log.txt"))
            log.addHandler(fh)
        if a["optimizer"] != "sgd":              # (the default run's log is what it always was)
            log.info(optimizer_line(a))
        model = _run(a, snapshot_path, ctx, log)
        ctx.barrier()
    finally:                    # also when the loop raises: leave the process groups, and a later train() in this process must not log into this file
        ctx.close()
        if fh is not None:
            log.removeHandler(fh)
            fh.close()
    return model


def _run(a, snapshot_path, ctx, log):
    device = ctx.device
    if ctx.group is not None:
        torch.cuda.set_device(device)
    torch.manual_seed(a["seed"])
    np.random.seed(a["seed"])                   # on every rank: ONE BCP box per iteration for the global batch, as the reference draws one per iteration
    make = lambda: net_factory(net_type=a["model"], in_chns=1, class_num=a["num_classes"], device=device, args=a)      # :240
    model = make()
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
    if a["mean_teacher"]:                                                        # ema_model = create_model(ema=True) (:238-251)
        teacher = build_teacher(make).eval()
        step = ChapStep(model, a, teacher=teacher, **step_kw)
    else:
        teacher, step = None, ChapStep(model, a, **step_kw)
    attach_step(ctx, step, a)                   # (data-parallel) rank 0's weights everywhere, the gradient exchange, the rank's noise stream
    loader = a.get("trainloader")
    if loader is None and a.get("root_path") and a.get("labeled_slices"):
        from .data import DeviceLoader, SliceStore
        store = SliceStore.from_h5_dir(a["root_path"], "train", device)
        n_lab = int(a["labeled_slices"])
        loader = DeviceLoader(store, range(n_lab), range(n_lab, len(store)), a["batch_size"], a["labeled_bs"], a["image_size"], a["seed"],
                              rank=ctx.rank, world=ctx.world)
    loader = loader or _synthetic_loader(a, ctx.rank)
    device_fed = a["use_graph"] and hasattr(loader, "next_into")      # the next batch is built on the device, beside the running iteration
    val = a.get("val_volumes")
    if val is None:
        vi, vl = synthetic_batch(a["seed"] + 4242, 8, 0, *a["image_size"], a["num_classes"])
        val = [(vi[:, 0].unsqueeze(0), vl.unsqueeze(0))]
    best, ema_best, captured = 0.0, -1.0, False         # (the first validated teacher is the best so far, whatever it scores)

    def validate(net):
        # each rank scores its shard of the volumes; the sum runs over the gathered values in volume order (one process: over all of them, as ever)
        per = [np.array(test_single_volume(im, lb, net, classes=a["num_classes"], patch_size=a["image_size"],
                                           model_type="logit_ensemble", device=device)) for im, lb in ctx.shard(val)]
        metric = sum(ctx.gather_in_order(per, len(val))) / len(val)
        return float(np.mean(metric, axis=0)[0]), float(np.mean(metric, axis=0)[1])

    def batches():
        """The epoch loop of the reference (:299-302, 459-463): `max_epoch = max_iterations // len(trainloader) + 1` passes
        over the loader, i.e. a finite loader is re-iterated until max_iterations is reached (the generator of the synthetic
        stand-in never ends; a one-shot iterator that runs dry ends the run, loudly)."""
        while True:
            n = 0
            for b in loader:
                n += 1
                yield b
            if n == 0:
                raise RuntimeError("chap_amd.train: the train loader yielded no batch (exhausted one-shot iterator or empty dataset) "
                                   "at iteration %d of %d" % (step.iter_num, a["max_iterations"]))

    gen = batches()
    sampled_batch = next(gen)
    while True:
        if a["use_graph"]:
            if not captured:
                step.capture(sampled_batch["image"].to(device), sampled_batch["label"].to(device))
                captured = True
                step.stage(sampled_batch["image"], sampled_batch["label"])
            out = step.replay()                      # the staged batch (host -> device copy done beside the previous iteration)
        else:
            out = step.step(sampled_batch["image"].to(device, non_blocking=True), sampled_batch["label"].to(device, non_blocking=True))
        it = step.iter_num
        if it % 50 == 0:                                                         # (:404 logs every iteration: a host sync each)
            log.info("iteration %d : bcp loss : %f vat loss : %f" % (it, sum(float(l[2]) for l in out["mix_losses"]), float(out["vat_loss"])))
        if "teacher_loss" in out and (it % 50 == 0 or it >= a["max_iterations"]):      # only with teacher_consistency > 0 (the default run's log is what it always was); the last iteration closes the record
            if "teacher_certain" in out:       # teacher_uncertainty > 0: the share of pixels the term counted, and the entropy threshold of this iteration
                log.info("iteration %d : teacher loss : %f : certain share : %f : entropy threshold : %f" % (
                    it, float(out["teacher_loss"]), float(out["teacher_certain"]) / step.teacher_pixels, uncertainty_threshold(it - 1, a)))
            else:
                log.info("iteration %d : teacher loss : %f" % (it, float(out["teacher_loss"])))
        if it > 0 and it % a["val_interval"] == 0:                               # :407-456
            sync_for_validation(ctx, step)       # (data-parallel) replicas equal, else raise; rank 0's BatchNorm statistics into every replica
            model.eval()
            performance, mean_hd95 = validate(model)
            # the checkpoint gate, on every rank (the replicas are equal: the same decision everywhere): no file is overwritten with a non-finite model
            check_finite_before_save(model.state_dict(), "the model", it)
            if ctx.is_main:
                torch.save(model.state_dict(), os.path.join(snapshot_path, "latest.pth"))
            if performance > best:              # the same decision on every rank: `performance` is the same word everywhere
                best = performance
                if ctx.is_main:
                    torch.save(model.state_dict(), os.path.join(snapshot_path, "{}_best_model.pth".format(a["model"])))
                    with open(os.path.join(snapshot_path, "val.csv"), "a", newline="") as f:
                        csv.writer(f).writerow([time.strftime("%Y-%m-%d %H:%M:%S"), it, round(best, 4)])
            log.info("iteration %d : model1_mean_dice : %f model1_mean_hd95 : %f" % (it, performance, mean_hd95))      # :453-454
            if teacher is not None:             # the averaged weights with the student's current BatchNorm statistics, after the student, same function
                step.sync_teacher_stats()
                ema_dice, ema_hd95 = validate(teacher)
                check_finite_before_save(teacher.state_dict(), "the mean teacher", it)
                if ctx.is_main:
                    torch.save(teacher.state_dict(), os.path.join(snapshot_path, "ema_latest.pth"))
                if ema_dice > ema_best:
                    ema_best = ema_dice
                    if ctx.is_main:
                        torch.save(teacher.state_dict(), os.path.join(snapshot_path, "{}_ema_best_model.pth".format(a["model"])))
                log.info("iteration %d : ema_mean_dice : %f ema_mean_hd95 : %f" % (it, ema_dice, ema_hd95))
            model.train()
            ctx.barrier()                       # no rank runs ahead of a half-written checkpoint
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
    return model
