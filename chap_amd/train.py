"""Host side of one CHAP training iteration, mirroring code/train_ours_2D.py:301-389 step by step
(same names where the reference has them).  Every tensor op is a libchap_hip.so kernel; torch
provides memory, streams, the autograd trampoline for the two network nodes and (optionally) HIP
graph capture of the whole iteration.

Pieces that are ABSENT from the reference (losses.VAT2d, patch.create_maskV1, losses.DiceLoss_bcp,
ramps.sigmoid_rampup) follow the definitions in DESIGN.md (P1-P4); the CPU oracle restates the same
definitions (oracle/train_step.py).
"""
import contextlib
import math
import os

import numpy as np
import torch

from . import ops
from .engine import switch


def sigmoid_rampup(current, rampup_length):
    if rampup_length == 0:
        return 1.0
    t = float(np.clip(current, 0.0, rampup_length)) / rampup_length
    return float(math.exp(-5.0 * (1.0 - t) ** 2))


def get_current_consistency_weight(epoch, args):            # train_ours_2D.py:34-36
    return args["consistency"] * sigmoid_rampup(epoch, args["consistency_rampup"])


DEFAULT_ARGS = dict(base_lr=0.01, batch_size=24, labeled_bs=12, max_iterations=30000, num_classes=4,
                    consistency=1.0, consistency_rampup=50.0, noise_mag=10.0, epi=6.0, topk1=0.1,
                    adv_noise=True, adv_losstype="kl", vat_iters=1, vat_sign=False, nms=1,
                    momentum=0.9, weight_decay=1e-4, dropout=False, comp_drop=False,
                    teacher_consistency=0.0, teacher_noise=0.1,
                    teacher_uncertainty=0, uncertainty_threshold=(0.75, 1.0))


def ema_alpha(global_step, decay):
    """alpha = min(1 - 1 / (global_step + 1), decay) (update_ema_variables, train_ours_2D.py:52), in double: 0 at step 0 (the average starts
    as a copy of the weights), the plain mean of the weights seen so far during the first 1 / (1 - decay) steps, `decay` from then on."""
    return min(1.0 - 1.0 / (global_step + 1), decay)


def ema_coefficients(global_step, decay):
    """(a, b) of ema = a * ema + b * param as the kernel reads them: alpha and 1 - alpha, each rounded to fp32 on its own."""
    alpha = ema_alpha(global_step, decay)
    f = lambda v: float(torch.tensor(v, dtype=torch.float64).float())
    return f(alpha), f(1.0 - alpha)


def build_teacher(factory):
    """ema_model = create_model(ema=True) (train_ours_2D.py:238-251): `factory()` -- the call that built the student -- run on a FORK of the torch
    (host and device), numpy and Python RNG states, which are put back afterwards: the student's run draws the numbers it draws without a
    teacher.  What the teacher is initialised with does not matter: the first optimizer step overwrites it with the student's weights (alpha = 0)."""
    import random
    np_state, py_state = np.random.get_state(), random.getstate()
    devices = [torch.cuda.current_device()] if torch.cuda.is_available() else []
    try:
        with torch.random.fork_rng(devices=devices):
            teacher = factory()
    finally:
        np.random.set_state(np_state)
        random.setstate(py_state)
    for p in teacher.parameters():
        p.requires_grad_(False)                 # param.detach_() (:243-244)
    return teacher


class FusedOptimizer:
    """What the optimizers of the captured step share: the flat parameter buffer of `model`, the learning rate as a word in device memory
    (graph replays pick up new values; ChapStep moves it into its schedule block), the mean teacher's average and the gradient guard.
    A subclass allocates its state and issues its kernels in step(); state_tensors() lists that state (what data-parallel replicas compare)
    and state_dict() / load_state_dict() carry it through a checkpoint, tagged with `kind`."""

    kind = None

    def __init__(self, model, lr, ema=None, ema_decay=0.99, guard=None):
        self.model = model
        flat = model.flat_buffers()[0]
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=flat.device)
        self.param_groups = [{"lr": float(lr)}]
        self.ema, self.ema_decay, self.ema_coef, self.ema_model = None, float(ema_decay), None, None
        if ema is not None:
            self.set_ema(ema)
        self.guard = None
        if guard is not None:
            self.set_guard(guard)

    def set_guard(self, guard):
        """None detaches it: step() is the unguarded launch again."""
        flat = self.model.flat_buffers()[0]
        if guard is not None and (guard.ws is None or guard.ws.device != flat.device):
            raise ValueError("chap_amd %s: the guard lives on %s, the parameters on %s" % (type(self).__name__, guard.device, flat.device))
        self.guard = guard

    def set_ema(self, ema, model=None):
        """`model`: the module whose parameters are views of `ema` (its packed weight copies go stale with every step)."""
        flat = self.model.flat_buffers()[0]
        if ema.dtype != torch.float32 or ema.shape != flat.shape or ema.device != flat.device or not ema.is_contiguous():
            raise ValueError("chap_amd %s: ema must be a contiguous fp32 tensor of the flat parameter buffer's shape %s on %s, got %s %s on %s"
                             % (type(self).__name__, tuple(flat.shape), flat.device, ema.dtype, tuple(ema.shape), ema.device))
        self.ema, self.ema_model = ema, model
        if self.ema_coef is None:
            self.ema_coef = torch.tensor([0.0, 1.0], dtype=torch.float32, device=flat.device)

    def set_ema_step(self, global_step):
        a, b = ema_coefficients(global_step, self.ema_decay)
        self.ema_coef.copy_(torch.tensor([a, b], dtype=torch.float32))

    def set_lr(self, lr):
        self.param_groups[0]["lr"] = float(lr)
        self.lr_dev.fill_(float(lr))

    def zero_grad(self, set_to_none=False):
        pass                                   # the step kernel zeroes the gradient buffer

    def state_tensors(self):
        raise NotImplementedError

    def state_dict(self):
        raise NotImplementedError

    def _check_kind(self, st):
        got = st.get("kind") if isinstance(st, dict) else None
        if got != self.kind:
            raise ValueError("chap_amd %s: the optimizer state is of kind %r, this optimizer's is %r" % (type(self).__name__, got, self.kind))


class FusedSGD(FusedOptimizer):
    """optim.SGD(lr, momentum=0.9, weight_decay=1e-4) (train_ours_2D.py:278) as ONE kernel over the
    model's flat parameter buffer; lr lives in device memory (graph replays pick up new values).

    `ema` (a flat fp32 tensor of the parameter buffer's size: the mean teacher's parameters): the same launch also averages the weights
    into it, ema = a * ema + b * param (update_ema_variables, :50-54), with (a, b) = `ema_coef`, two fp32 words in device memory that
    set_ema_step() -- or the owner of the words, ChapStep's schedule block -- fills before every step.

    `guard` (chap_amd.guard.StepGuard): step() first takes the norm of the gradient it is about to apply (chap_grad_norm) and then issues the
    guarded form of the same kernel, which reads the clip coefficient and the skip flag from the guard's state block."""

    kind = "sgd"

    def __init__(self, model, lr, momentum=0.9, weight_decay=1e-4, ema=None, ema_decay=0.99, guard=None):
        self.momentum, self.weight_decay = momentum, weight_decay
        self.mom = torch.zeros_like(model.flat_buffers()[0])
        super().__init__(model, lr, ema, ema_decay, guard)

    def state_tensors(self):
        return [self.mom]

    def state_dict(self):
        return {"kind": "sgd", "momentum": self.mom.detach().clone()}

    def load_state_dict(self, st):
        self._check_kind(st)
        self.mom.copy_(st["momentum"])

    def step(self, grad_scale=1.0, grad2=None):
        flat, grad = self.model.flat_buffers()
        if self.guard is not None:              # behind the gradient exchange: the norm of what is applied, the same word on every rank
            self.guard.launch_norm(grad, grad2, grad_scale)
            ops.sgd_guard_step(flat, grad, self.mom, self.lr_dev, self.momentum, self.weight_decay, self.guard.state, self.ema, self.ema_coef, grad_scale, True, grad2)
            if self.ema_model is not None:
                self.ema_model.mark_params_dirty()
        elif self.ema is None:
            ops.sgd_step(flat, grad, self.mom, self.lr_dev, self.momentum, self.weight_decay, grad_scale, True, grad2)
        else:
            ops.sgd_ema_step(flat, grad, self.mom, self.lr_dev, self.momentum, self.weight_decay, self.ema, self.ema_coef, grad_scale, True, grad2)
            if self.ema_model is not None:
                self.ema_model.mark_params_dirty()
        self.model.mark_params_dirty()


class FusedAdamW(FusedOptimizer):
    """torch.optim.AdamW(lr, betas, eps, weight_decay) -- `decoupled=False`: torch.optim.Adam with its L2 weight decay -- over the model's flat
    parameter buffer, as two launches (include/chap_hip_optim.h): chap_adam_tick advances the step counter t and forms lr / (1 - beta1^t),
    sqrt(1 - beta2^t) and 1 - lr * weight_decay in a 16-byte state block in device memory, chap_adam_step is the streaming update that reads
    them.  The counter lives on the device: a replayed graph needs no host upload, and a step the guard skips does not count (torch's t when
    step() is not called).  `ema` and `guard` as FusedSGD's: the average is part of the same launch, the clip coefficient and the skip flag are
    read from the guard's state block.  No AMSGrad, one group of hyper-parameters for all parameters."""

    kind = "adam"

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True, ema=None, ema_decay=0.99, guard=None):
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError("chap_amd FusedAdamW: betas=%r, need 0 <= beta < 1" % (tuple(betas),))
        if not eps > 0.0:
            raise ValueError("chap_amd FusedAdamW: eps=%r, need eps > 0" % (eps,))
        self.betas, self.eps, self.weight_decay, self.decoupled = (b1, b2), float(eps), float(weight_decay), bool(decoupled)
        flat = model.flat_buffers()[0]
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
        self.state = torch.zeros(ops.ADAM_STATE_WORDS, dtype=torch.int32, device=flat.device)       # chap_adam_state
        super().__init__(model, lr, ema, ema_decay, guard)

    def state_tensors(self):
        return [self.exp_avg, self.exp_avg_sq, self.state]

    def state_dict(self):
        return {"kind": "adam", "exp_avg": self.exp_avg.detach().clone(), "exp_avg_sq": self.exp_avg_sq.detach().clone(),
                "state": self.state.detach().clone()}

    def load_state_dict(self, st):
        self._check_kind(st)
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])
        self.state.copy_(st["state"])

    def step(self, grad_scale=1.0, grad2=None):
        flat, grad = self.model.flat_buffers()
        gs = None
        if self.guard is not None:              # behind the gradient exchange, as FusedSGD.step
            self.guard.launch_norm(grad, grad2, grad_scale)
            gs = self.guard.state
        ops.adam_tick(self.state, self.lr_dev, self.betas[0], self.betas[1], self.weight_decay, self.decoupled, gs)
        ops.adam_step(flat, grad, self.exp_avg, self.exp_avg_sq, self.state, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.decoupled,
                      self.ema, self.ema_coef if self.ema is not None else None, gs, grad_scale, True, grad2)
        if self.ema_model is not None:
            self.ema_model.mark_params_dirty()
        self.model.mark_params_dirty()


OPTIMIZERS = ("sgd", "adam", "adamw")


def check_optimizer(name, who="chap_amd"):
    """The optimizers the train() entries build.  They call this before anything is allocated or written."""
    if name not in OPTIMIZERS:
        raise ValueError("%s: optimizer=%r; choose one of %s" % (who, name, ", ".join(OPTIMIZERS)))


def optimizer_line(args):
    """The line of log.txt that names an Adam run's optimizer and its hyper-parameters (a default run's log is what it always was: no line)."""
    name = args["optimizer"]
    b = args.get("betas", (0.9, 0.999))
    return "optimizer %s: base_lr %g, betas (%g, %g), eps %g, weight_decay %g (%s)" % (
        name, args["base_lr"], b[0], b[1], args.get("adam_eps", 1e-8), args.get("weight_decay", 1e-4), "decoupled" if name == "adamw" else "L2")


def check_teacher_consistency(args, have_teacher, who="chap_amd"):
    """args['teacher_consistency'] (0 = off: the mean teacher is only averaged) and args['teacher_noise'].  The term needs a teacher to run; the
    train() entries and ChapStep call this before anything is allocated or written."""
    w, noise = float(args.get("teacher_consistency", 0.0)), float(args.get("teacher_noise", 0.1))
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError("%s: teacher_consistency=%r, need a finite weight >= 0" % (who, args.get("teacher_consistency")))
    if w > 0.0 and not have_teacher:
        raise ValueError("%s: teacher_consistency=%g needs the mean teacher (mean_teacher=True / ChapStep(teacher=...)): its predictions are the target" % (who, w))
    if w > 0.0 and not (math.isfinite(noise) and noise >= 0.0):
        raise ValueError("%s: teacher_noise=%r, need a finite magnitude >= 0" % (who, args.get("teacher_noise")))
    return w


def check_teacher_uncertainty(args, who="chap_amd"):
    """args['teacher_uncertainty'] (0 = off, or T = 1..8 noisy teacher passes whose mean prediction's entropy masks the consistency term) and
    args['uncertainty_threshold'] = (lo, hi), fractions of ln C with 0 < lo <= hi.  T > 0 needs the term itself (teacher_consistency > 0, hence
    the teacher).  Called where check_teacher_consistency is, before anything is allocated or written.  -> T"""
    T = args.get("teacher_uncertainty", 0)
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or not 0 <= T <= 8:
        raise ValueError("%s: teacher_uncertainty=%r, need 0 (off) or the number of noisy teacher passes T = 1..8" % (who, T))
    T = int(T)
    if T == 0:
        return 0
    if not float(args.get("teacher_consistency", 0.0)) > 0.0:
        raise ValueError("%s: teacher_uncertainty=%d needs teacher_consistency > 0: it masks that term" % (who, T))
    thr = args.get("uncertainty_threshold", (0.75, 1.0))
    try:
        lo, hi = (float(v) for v in thr)
    except (TypeError, ValueError):
        raise ValueError("%s: uncertainty_threshold=%r, need two fractions (lo, hi) of ln C" % (who, thr))
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError("%s: uncertainty_threshold=%r, need finite fractions of ln C with 0 < lo <= hi" % (who, thr))
    return T


def uncertainty_threshold(iter_num, args):
    """thr(iter) = (lo + (hi - lo) * sigmoid_rampup(iter, max_iterations)) * ln C: the uncertainty-aware mean teacher's
    (0.75 + 0.25 * ramp) * ln 2, for C classes."""
    lo, hi = (float(v) for v in args.get("uncertainty_threshold", (0.75, 1.0)))
    return (lo + (hi - lo) * sigmoid_rampup(iter_num, args["max_iterations"])) * math.log(args["num_classes"])


def build_optimizer(model, args):
    """args['optimizer']: 'sgd' (default) -> FusedSGD(base_lr, momentum, weight_decay); 'adam' / 'adamw' -> FusedAdamW(base_lr, betas, adam_eps,
    weight_decay) with L2 / decoupled weight decay."""
    name = args.get("optimizer", "sgd")
    check_optimizer(name)
    if name == "sgd":
        return FusedSGD(model, args["base_lr"], args["momentum"], args["weight_decay"])
    return FusedAdamW(model, args["base_lr"], tuple(args.get("betas", (0.9, 0.999))), args.get("adam_eps", 1e-8), args["weight_decay"],
                      decoupled=(name == "adamw"))


def _distinct_streams(dev, n):
    """n streams with pairwise different handles, none of them the current or the default stream."""
    seen = {0, torch.cuda.current_stream(dev).cuda_stream}
    out = []
    for _ in range(256):
        s = torch.cuda.Stream(device=dev)
        if s.cuda_stream not in seen:
            seen.add(s.cuda_stream)
            out.append(s)
            if len(out) == n:
                return out
    raise RuntimeError("chap_amd: could not get %d distinct streams from the pool" % n)


def check_graph_environment(concurrent=True, environ=None):
    """Refuse a graph capture the runtime is known to die in.  The captured iteration forks four streams (capture origin, pass B, second decoder,
    early VAT pass); with GPU_MAX_HW_QUEUES below 3 the FIRST REPLAY of any such graph aborts inside the ROCm 7.2 runtime with no HIP error
    (profiles/r03_runtime_aborts.log: 2D and 3D, default schedule) -- a user-reachable environment, so capture() raises here instead.  A
    single-stream iteration (ChapStep(args={'concurrent': False})) captures as one chain and is not affected."""
    from ._lib import ChapError
    env = os.environ if environ is None else environ
    v = env.get("GPU_MAX_HW_QUEUES")
    if v is None or not concurrent:
        return
    try:
        n = int(v)
    except ValueError:
        return
    if n < 3:
        raise ChapError("chap_amd: GPU_MAX_HW_QUEUES=%d: the multi-stream HIP graph of the iteration needs at least 3 hardware queues (its first replay "
                        "aborts in the runtime below that).  Unset GPU_MAX_HW_QUEUES (default 4) or build the step with args={'concurrent': False}." % n)


# The passes on a capture's origin stream that may fork their second decoder onto a stream of its own, as the bits of CHAP_FORK_MASK (engine.SWITCHES)
FORK_PASS_A = 1                 # pass A
FORK_POWER_BACKWARD = 2         # the power iteration's backward to the input
FORK_VAT_FORWARD = 4            # the VAT forward passes after the first
FORK_FINAL_BACKWARD = 8         # the final VAT backward


def check_num_classes(nc, who="chap_amd"):
    """The class counts the training kernels are built for (ops.LOSS_CLASSES: csrc/loss.hip instantiates 2..8; the shared totals arrays, the
    inference kernels and the V-Net head route end at 8).  The train() entries call this before anything is allocated."""
    if nc not in ops.LOSS_CLASSES:
        raise ValueError("%s: num_classes=%r; the training kernels are built for %d to %d classes" % (who, nc, ops.LOSS_CLASSES[0], ops.LOSS_CLASSES[-1]))


class VAT2d:
    """adv_loss = VAT2d(xi, epi, num_classes); adv_loss(model, x, soft1, soft2, mask, losstype)
    (call sites train_ours_2D.py:290,372); losstype 'kl' or 'dice' (--adv_losstype, :515), `sign=True` = the FGSM-style
    sign step  r = epi / sqrt(P) * sign(d) * mask.  Returns a 1-element device tensor; the gradient of
    `weight * loss` w.r.t. the parameters is accumulated into the model's gradient buffer here
    (the network node is driven directly with d(loss)/d(logits) from the fused KL kernel)."""

    def __init__(self, xi=10.0, epi=6.0, num_classes=4, ip=1, sign=False):
        self.xi, self.epi, self.num_classes, self.ip, self.sign = xi, epi, num_classes, ip, sign

    def begin(self, model, x, U, inject=None):
        """The part of the VAT computation that does NOT depend on pass A: the initial direction d (U(-.5,.5), per-sample L2
        normalised) and the forward pass of the first power iteration on x + xi * d.  ChapStep runs it on a stream of its own
        BESIDE pass A (the two forwards only meet in the distance kernel), which takes one forward pass off the critical chain
        of the iteration.  Returns the state for finish()."""
        inject = inject or {}
        x = x[-U:].contiguous()                 # "perturb the last U samples" (SURVEY.md section 3.1 note)
        d = torch.empty_like(x)
        if inject.get("d0") is not None:
            ops.l2_normalize(inject["d0"], d)
        else:
            ops.rand_uniform(d, model._rng.next_seed(), -0.5, 0.5, seed_dev=model._rng.seed_dev)
            ops.l2_normalize(d, d)
        xh = torch.empty_like(x).requires_grad_(True)
        first = None
        if self.ip > 0:
            ops.perturb(x, d, xh, self.xi)
            with model.frozen():
                first = model(xh, update_stats=False, drop_masks=inject.get("drop_V0"))
        return dict(x=x, d=d, xh=xh, first=first, inject=inject)

    def finish(self, model, st, soft1, soft2, mask, losstype="kl", weight_dev=None, accumulate_grad=True, grad_buffer=None, weight=1.0, forks=None):
        """The rest of the VAT computation, pass by pass: [power iteration k: distance gradient, backward to the input, normalise] ..., the final forward +
        distance, the final backward.  `forks(bit)` (ChapStep._forks; default: nothing) is entered around every pass: which of them fork their second
        decoder under capture (FORK_*, CHAP_FORK_MASK).  Returns the loss."""
        if losstype not in ops.DIST_MODES:
            raise ValueError("chap_amd VAT2d: adv_losstype=%r (--adv_losstype {kl,dice}, train_ours_2D.py:515)" % (losstype,))
        forks = forks or (lambda bit: contextlib.nullcontext())
        x, d, xh, inject = st["x"], st["d"], st["xh"], st["inject"]
        for it in range(self.ip):
            if it == 0:
                l1, l2 = st["first"]
            else:
                ops.perturb(x, d, xh, self.xi)
                with forks(FORK_VAT_FORWARD), model.frozen():
                    l1, l2 = model(xh, update_stats=False, drop_masks=inject.get("drop_V%d" % it))
            g1, g2 = torch.empty_like(l1), torch.empty_like(l2)
            ops.kl_fwd_bwd((l1, l2), (soft1, soft2), None, (g1, g2), mode=losstype)
            # d(distance)/d(x) only (the weights are frozen: no weight-gradient kernels), on the CURRENT stream whatever stream the
            # forward ran on (torch.autograd would run the node on the forward's stream)
            with forks(FORK_POWER_BACKWARD):
                dx = model.backward_saved(l1, [g1, g2], need_wgrad=False, need_dx=True)
            model.release_saved(l1)
            ops.l2_normalize(dx, d)
        xa = torch.empty_like(x)
        m = None if mask is None else mask.reshape(x.shape)
        alpha = self.epi / math.sqrt(x[0].numel()) if self.sign else self.epi
        ops.perturb(x, d, xa, alpha, mask=m, sign=self.sign)
        loss = torch.zeros(1, dtype=torch.float32, device=x.device)
        if accumulate_grad:
            with forks(FORK_VAT_FORWARD):
                l1, l2 = model(xa, update_stats=False, drop_masks=inject.get("drop_VF"), grad_buffer=grad_buffer)
            g1, g2 = torch.empty_like(l1), torch.empty_like(l2)
            ops.kl_fwd_bwd((l1, l2), (soft1, soft2), loss, (g1, g2), gscale=weight, gscale_dev=weight_dev, mode=losstype)
            with forks(FORK_FINAL_BACKWARD):
                torch.autograd.backward([l1, l2], [g1, g2])
        else:
            with forks(FORK_VAT_FORWARD), torch.no_grad():
                l1, l2 = model(xa, update_stats=False, drop_masks=inject.get("drop_VF"))
            ops.kl_fwd_bwd((l1, l2), (soft1, soft2), loss, mode=losstype)
        return loss

    def __call__(self, model, x, soft1, soft2, mask, losstype="kl", weight_dev=None, inject=None, accumulate_grad=True, grad_buffer=None,
                 weight=1.0):
        st = self.begin(model, x, soft1.shape[0], inject)
        return self.finish(model, st, soft1, soft2, mask, losstype, weight_dev, accumulate_grad, grad_buffer, weight)


class GradSim:
    """gradsim = grad.GradSim(device, num_classes, dir) (ABSENT upstream; call sites train_ours_2D.py:288,297,360,365): the
    channel scores of the channel-level perturbation.  Definition of this build (parity unpinned): for each of
    the five encoder levels, the conv kernel that produces the level's feature (the second conv of its ConvBlock) and, per
    output channel, the cosine similarity of the gradients of the LABELED part and of the UNLABELED part of the BCP loss
    (loss_l, loss_u at train_ours_2D.py:352-353) with respect to that kernel -- channels on which the two supervisions agree
    score high and are kept more often (scores_dropoutV2, FilterDropout.py:116-138).

        init_simsocre() -> [zeros(C_l)]          (:297; all-zero scores = the Dropout2d pair, FilterDropout.py:71-73)
        get_sim()       -> the current scores     (:360)
        get_grad_convkernel(grad_l, grad_u, model, optimizer=None, iter_num=0) -> the new scores   (:365)

    Difference to the call site: upstream hands over the two LOSSES (autograd); here the caller hands over the two flat
    gradient buffers (model layout) that its two backward passes filled."""

    KEYS_2D = ["encoder.in_conv.conv_conv.4.weight"] + ["encoder.down%d.maxpool_conv.1.conv_conv.4.weight" % i for i in range(1, 5)]

    def __init__(self, device, num_classes=4, dir=None, ema=0.0):
        self.device, self.num_classes, self.dir, self.ema = device, num_classes, dir, ema
        self.scores = None

    def init_simsocre(self, model=None):
        chans = (16, 32, 64, 128, 256) if model is None else [dict(model.named_parameters())[k].shape[0] for k in self.KEYS_2D]
        self.scores = [torch.zeros(c, dtype=torch.float32, device=self.device) for c in chans]
        return self.scores

    def get_sim(self):
        if self.scores is None:
            self.init_simsocre()
        return self.scores

    def get_grad_convkernel(self, grad_l, grad_u, model, optimizer=None, iter_num=0):
        vl, vu = model.grad_views_of(grad_l), model.grad_views_of(grad_u)
        for sc, k in zip(self.get_sim(), self.KEYS_2D):
            ops.grad_sim(vl[k], vu[k], sc, self.ema)
        return self.scores


class ChapStep:
    """One iteration of train() (train_ours_2D.py:301-389) for a DualDecoder on 2D slices, or -- the
    same loop restated on 5-D tensors, the reference has no 3D training script -- a DualDecoder3d on
    volumes (cuboid BCP box, 26-connected largest component, in-plane 4x4 patches for the VAT mask).

    step(volume_batch [B,1,*sp] fp32, label_batch [B,*sp] int64) -> dict of device scalars.
    The BCP box offsets, LR and consistency weight live in device memory so that the whole iteration
    can be captured once as a HIP graph (`capture()`) and replayed."""

    MONITOR_LAYOUT = "chap"         # what the scalar words of a monitor row hold (chap_amd.monitor.SCALAR_LAYOUTS)

    def __init__(self, model, args=None, optimizer=None, world_size=1, teacher=None, monitor=None, guard=None):
        a = dict(DEFAULT_ARGS)
        a.update(args or {})
        self.args, self.model = a, model
        # weight of the mean teacher's consistency term (0: the teacher is averaged and never run, the step is launch for launch the one without the argument)
        self.teacher_w = check_teacher_consistency(a, teacher is not None, "chap_amd %s" % type(self).__name__)
        # T noisy teacher passes behind the term's entropy mask (0: the plain term, launch for launch)
        self.teacher_T = check_teacher_uncertainty(a, "chap_amd %s" % type(self).__name__)
        self.opt = optimizer or build_optimizer(model, a)
        self.adv_loss = VAT2d(xi=a["noise_mag"], epi=a["epi"], num_classes=a["num_classes"], ip=a["vat_iters"], sign=a["vat_sign"])
        dev = self.opt.lr_dev.device
        self.dims = getattr(model, "dims", 2)
        # host-scheduled values of an iteration in ONE device word block -> one host-to-device copy per step:
        # [BCP box: 4 / 6 int32 | consistency weight f32 | learning rate f32], and with a mean teacher [| a f32 | b f32] of its average behind them,
        # and with a monitor [| ring slot int32 | iteration int32] of the row its finalize kernel writes behind those, and with teacher_uncertainty
        # [| entropy threshold f32] behind everything else
        nbox = 4 if self.dims == 2 else 6
        self.teacher = teacher
        nsched = 8 if teacher is None else 10
        self.monitor = monitor
        if monitor is not None:
            if monitor.C != a["num_classes"] or monitor.ws is None or monitor.ws.device != dev:
                raise ValueError("chap_amd ChapStep: the monitor was built for %d classes on %s, the step runs %d on %s" % (monitor.C, monitor.device, a["num_classes"], dev))
            monitor.scalar_layout = self.MONITOR_LAYOUT
            self._mon_at = nsched
            nsched += 2
        if self.teacher_T > 0:      # [| entropy threshold f32] of the uncertainty mask, appended: no other word moves
            self._thr_at = nsched
            nsched += 1
        self._sched = torch.zeros(nsched, dtype=torch.int32, device=dev)
        self._sched_pin = [torch.empty(nsched, dtype=torch.int32).pin_memory() for _ in range(4)]      # host side of the schedule block (see _upload_sched)
        self._sched_ev, self._sched_k = [None] * 4, 0
        self.box = self._sched[:nbox]
        self.cw_dev = self._sched[6:7].view(torch.float32)
        self.teacher_pixels = 0
        self.thr_dev = self._sched[self._thr_at:self._thr_at + 1].view(torch.float32) if self.teacher_T > 0 else None
        if isinstance(self.opt, FusedOptimizer):                 # the optimizer reads its lr from the same block
            self._sched[7:8].view(torch.float32).copy_(self.opt.lr_dev)
            self.opt.lr_dev = self._sched[7:8].view(torch.float32)
        if teacher is not None:
            self._attach_teacher(teacher)
        self.guard = guard
        if guard is not None:
            if not isinstance(self.opt, FusedOptimizer):
                raise ValueError("chap_amd ChapStep: a gradient guard needs the fused optimizer (FusedSGD): clip and skip are part of that kernel")
            self.opt.set_guard(guard)
        self.iter_num = 0
        self.world_size = world_size
        self.grad_sync = None                   # parallel.DataParallelSync (world_size > 1)
        self._graph, self._graph_opt, self._graphs_dp = None, None, None
        # --dropout: per-level channel scores [C_l] = gradsim.get_sim() (train_ours_2D.py:360), refreshed every iteration by
        # gradsim.get_grad_convkernel (:365); all-zero (the initial value) = the Dropout2d pair (FilterDropout.py:71-73).
        # `sim_score` (or inject['sim_score']) overrides them.
        self.sim_score = None
        self.gradsim = None
        if a["dropout"] and self.dims == 2:
            self.gradsim = GradSim(dev, a["num_classes"])
            self.gradsim.init_simsocre(model)
            n_ = model.flat_buffers()[1].numel()
            self._grad_lu = torch.zeros(2 * n_, dtype=torch.float32, device=dev)      # gradients of loss_l | loss_u (pass B)
        # second gradient bucket: the VAT branch accumulates here, so it can run on its own stream beside the
        # BCP branch (and, data-parallel, its all-reduce overlaps); the fused SGD sums both buckets
        n = model.flat_buffers()[1].numel()
        self.grad_both = torch.zeros(2 * n, dtype=torch.float32, device=dev)     # [bucket 0 | bucket 1], one all-reduce
        model.swap_grad_buffer(self.grad_both[:n])
        self.grad2 = self.grad_both[n:]
        self.concurrent = bool(a.get("concurrent", True))
        # `passb_batch`: pass B's runs of small dependent launches as batched ones -- largest-CC over both heads' maps in one call, loss mask + BCP
        # mixing in one launch, the four mix_loss terms in one launch per kernel (bit-identical results, DESIGN.md section 5 "Pass B's
        # small launches").  On by default where pass B is a chain of its own beside the VAT chain (`concurrent`), the chain whose end is
        # the end of the step; the single-stream step keeps the separate calls unless the argument asks for the batched ones.
        pb = a.get("passb_batch")
        self.passb_batch = self.concurrent if pb is None else bool(pb)
        # Streams come from PyTorch's per-device pool (32 of them, handed out round-robin): two "new" streams of a long-lived
        # process can be the SAME stream.  The ones of an iteration must differ from each other and from the stream the graph is
        # captured on (pass B on the capture's origin stream would run behind the VAT chain, not beside it), so they are drawn
        # until they do and the capture gets a stream of its own.
        st = _distinct_streams(dev, 4)
        self._cap = st[3]                                          # origin stream of capture()
        self._side = st[0] if self.concurrent else None
        # Decoder-level concurrency inside a captured graph.  On ROCm 7.2 a captured stream may fork/join with the
        # capture's ORIGIN stream any number of times, but an event dependency between two forked streams crashes
        # hipStreamEndCapture.  So the long chain of the iteration (the VAT branch: K+1 forward/backward pairs)
        # stays on the origin stream, where the executor may fork its second decoder, and the short one (pass B)
        # goes to the side stream with its decoders back to back.
        self._d2 = st[1] if self.concurrent else None
        self._pre = st[2] if self.concurrent else None              # the VAT pre-pass beside pass A
        self._fork_sides, self._fork_mask = {}, 0                   # inside _decoder_fork under capture: {origin stream: forked stream}, CHAP_FORK_MASK
        self._stage_v, self._staged = None, False                   # stage() / stage_from(): made at the first call; a staged batch waits for replay()

    # ------------------------------------------------------------------ mean teacher (train_ours_2D.py:50-54, 238-251: built there, switched off)
    def _attach_teacher(self, teacher):
        """`teacher`: a second instance of the student's class, create_model(ema=True) (:238-245).  Its parameters never require grad (:243-244); its
        flat parameter buffer is what the optimizer kernel averages the student's weights into, with the coefficients in words 8-9 of the
        schedule block.  With args['teacher_consistency'] > 0 pass B runs it on a noised copy of its input and pulls the student towards its
        prediction (_teacher_pass); otherwise the iteration never runs it.  To evaluate it, call sync_teacher_stats() first."""
        model = self.model
        if not isinstance(self.opt, FusedOptimizer):
            raise ValueError("chap_amd ChapStep: a mean teacher needs the fused optimizer (FusedSGD): its average is part of that kernel")
        if teacher is model or type(teacher) is not type(model):
            raise ValueError("chap_amd ChapStep: the teacher must be a second instance of %s, got %s" % (type(model).__name__, type(teacher).__name__))
        for p in teacher.parameters():
            p.requires_grad_(False)
        teacher.set_compute_dtype(model.compute_dtype)
        model.flat_buffers()
        teacher._ensure_flat()
        if [(n, tuple(p.shape)) for n, p in teacher.named_parameters()] != [(n, tuple(p.shape)) for n, p in model.named_parameters()] or teacher._offsets != model._offsets:
            raise ValueError("chap_amd ChapStep: teacher and student differ in their parameters")
        self.opt.ema_decay = float(self.args.get("ema_decay", 0.99))
        self.opt.set_ema(teacher._flat, teacher)
        self._sched[8:10].view(torch.float32).copy_(torch.tensor([0.0, 1.0]))
        self.opt.ema_coef = self._sched[8:10].view(torch.float32)

    def sync_teacher_stats(self):
        """Copy the student's BatchNorm buffers (running_mean, running_var, num_batches_tracked) into the teacher, which also follows the student's
        compute dtype.  update_ema_variables averages PARAMETERS only and the reference never evaluates its ema model, so what statistics an
        evaluated teacher normalises with is this build's choice (DESIGN.md "Mean teacher"): the student's current ones.  Call before evaluating."""
        t = self.teacher
        if t is None:
            raise RuntimeError("chap_amd ChapStep: sync_teacher_stats() without a teacher")
        if t._flat is not self.opt.ema or not t._flat_ok():
            raise RuntimeError("chap_amd ChapStep: the teacher's parameters were moved off the buffer the optimizer averages into")
        t.set_compute_dtype(self.model.compute_dtype)
        src = dict(self.model.named_buffers())
        with torch.no_grad():
            for n, b in t.named_buffers():
                b.copy_(src[n])
        t.mark_params_dirty()

    # ------------------------------------------------------------------ host-side schedule values
    def prepare(self, box_yx=None):
        """Host work of an iteration that must happen BEFORE the device work (and outside a captured
        graph): BCP box offsets (np.random.randint, train_ours_2D.py:97-98), consistency weight."""
        a = self.args
        sizes = [int(s * 2 / 3) for s in self._hw]                 # patch = 2/3 of every side (:96)
        if box_yx is None:
            box_yx = tuple(np.random.randint(0, s - p) for s, p in zip(self._hw, sizes))
        self._upload_sched(list(box_yx) + sizes, get_current_consistency_weight(self.iter_num // 150, a))

    def _upload_sched(self, box_vals, cw):
        import struct
        f2i = lambda v: struct.unpack("<i", struct.pack("<f", float(v)))[0]
        vals = list(box_vals) + [0] * (6 - len(box_vals)) + [f2i(cw), f2i(self.opt.param_groups[0]["lr"])]
        if self.teacher is not None:            # global_step of update_ema_variables (train_ours_2D.py:50-54) = iter_num before finish() counts this step
            vals += [f2i(c) for c in ema_coefficients(self.iter_num, self.opt.ema_decay)]
        if self.monitor is not None:            # the row of this iteration: its ring slot, and the number the reference's log line prints (iter_num + 1, train_ours_2D.py:385,404-405)
            vals += [self.monitor.next_slot(), self.iter_num + 1]
        if self.teacher_T > 0:
            vals += [f2i(uncertainty_threshold(self.iter_num, self.args))]
        # Through a small ring of PINNED host blocks, asynchronously: a plain `copy_` from pageable memory synchronises the stream,
        # i.e. the host would wait for the previous iteration to drain before it even starts launching the next one (the GPU then
        # idles while the graph's first nodes are being submitted: ~0.5 ms of gaps at the head of every replay in the kernel trace).
        # A slot is reused only after the copy that last read it has run (event), which also bounds how far the host runs ahead.
        k = self._sched_k
        self._sched_k = (k + 1) % len(self._sched_pin)
        if self._sched_ev[k] is not None:
            self._sched_ev[k].synchronize()
        self._sched_pin[k].copy_(torch.tensor(vals, dtype=torch.int32))
        self._sched.copy_(self._sched_pin[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._sched_ev[k] = ev

    def finish(self):
        """poly LR applied AFTER the step (train_ours_2D.py:385-389)."""
        a = self.args
        self.iter_num += 1
        if self.monitor is not None:
            self.monitor.advance()
        lr_ = a["base_lr"] * (1.0 - self.iter_num / a["max_iterations"]) ** 0.9
        if isinstance(self.opt, FusedOptimizer):
            self.opt.param_groups[0]["lr"] = float(lr_)          # reaches the device with the next step's schedule block
        else:
            self.opt.set_lr(lr_)
        return lr_

    # ------------------------------------------------------------------ checkpoint / resume (build extension)
    def state_dict(self):
        """Everything a long run needs to continue exactly where it stopped.  'model' is the reference's checkpoint
        (what train_ours_2D.py:428-435 saves with torch.save(model.state_dict())); the rest is absent upstream:
        momentum buffer ('momentum'; with Adam 'optimizer' instead: its moments and state block), iteration counter (drives poly LR and the consistency ramp), numpy RNG state (BCP box
        offsets) and the dropout / VAT noise RNG epoch.  With a mean teacher: 'ema', its flat parameter buffer."""
        rng = self.model._rng
        st = {"model": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
                "iter_num": int(self.iter_num),
                "lr": float(self.opt.param_groups[0]["lr"]), "numpy_rng": np.random.get_state(),
                "rng": {"base": rng.base, "count": rng.count, "seed_dev": int(rng.seed_dev.item())},
                "gradsim": None if self.gradsim is None else [sc.detach().clone() for sc in self.gradsim.get_sim()]}
        if isinstance(self.opt, FusedOptimizer) and self.opt.kind != "sgd":     # Adam: both moments and the four words of its state block
            st["optimizer"] = self.opt.state_dict()
        else:                                   # SGD keeps the key it always had
            st["momentum"] = self.opt.mom.detach().clone()
        if self.teacher is not None:
            st["ema"] = self.opt.ema.detach().clone()
        if self.guard is not None:
            st["guard"] = self.guard.state_dict()
        return st

    def load_state_dict(self, st):
        if isinstance(self.opt, FusedOptimizer):         # before anything is changed: the checkpoint carries this optimizer's kind of state
            have = st["optimizer"].get("kind") if isinstance(st.get("optimizer"), dict) else ("sgd" if "momentum" in st else None)
            if have != self.opt.kind:
                raise ValueError("chap_amd ChapStep: the checkpoint carries optimizer state of kind %r, the step's optimizer (%s) needs %r"
                                 % (have, type(self.opt).__name__, self.opt.kind))
        self.model.load_state_dict(st["model"], strict=True)
        if isinstance(self.opt, FusedOptimizer):
            self.opt.load_state_dict(st["optimizer"] if self.opt.kind != "sgd" else {"kind": "sgd", "momentum": st["momentum"]})
        else:
            self.opt.mom.copy_(st["momentum"])
        self.iter_num = int(st["iter_num"])
        self.opt.set_lr(st["lr"])
        np.random.set_state(st["numpy_rng"])
        rng = self.model._rng
        rng.base, rng.count = int(st["rng"]["base"]), int(st["rng"]["count"])
        rng.seed_dev.fill_(int(st["rng"]["seed_dev"]))
        if self.gradsim is not None and st.get("gradsim") is not None:
            for dst, src in zip(self.gradsim.get_sim(), st["gradsim"]):
                dst.copy_(src)
        self.grad_both.zero_()
        if self.teacher is not None:            # a checkpoint of a run without a teacher: the average starts at the loaded weights
            ema = st.get("ema")
            self.opt.ema.copy_(self.model.flat_buffers()[0] if ema is None else ema)
            self.teacher.mark_params_dirty()
        if self.guard is not None and st.get("guard") is not None:      # a checkpoint of a run without a guard: the counters stay
            self.guard.load_state_dict(st["guard"])
        return self

    # ------------------------------------------------------------------ the device work
    def exchange_and_update(self):
        """(data-parallel) all-reduce of both gradient buckets, then optimizer.step() (:381-383): the fused SGD
        sums the buckets, scales by 1/world and zeroes them."""
        if self.grad_sync is not None:
            self.grad_sync.start()
            self.grad_sync.wait()
        self.opt.step(grad_scale=1.0 / self.world_size, grad2=self.grad2)

    def device_step(self, volume_batch, label_batch, inject=None, update=True):
        """The device work of one iteration on the current stream (+ the side streams): phase A (pass A, pseudo labels,
        perturbation mask), then phase B (largest-CC filter, BCP mixing, pass B forward / backward -> gradient bucket 0) on a
        side stream BESIDE phase V (the VAT chain -> bucket 1) on this one, then the gradient exchange and the optimizer."""
        with self.model.hold_stat_shift():          # one snapshot of the running means for all passes of the iteration (determinism)
            return self._iteration(volume_batch, label_batch, inject, update)

    def _iteration(self, volume_batch, label_batch, inject=None, update=True):
        main = torch.cuda.current_stream()
        with self._decoder_fork(main):
            ctx = self._phase_a(volume_batch, label_batch, inject)
            if self.concurrent and self.args["adv_noise"]:
                # Phase B (side stream) and phase V (this stream, the iteration's critical chain): all of phase B is issued first, then phase V.  Round 4 tried
                # issuing them pass by pass in alternation (same launches, same streams, bit-identical results): 8.05 ms per 2D step instead of 6.5 -- the
                # ROCm 7.2 graph executor places the chains of a captured graph on its hardware queues by the creation order of the nodes, and in that
                # order pass B lands on the VAT chain's queue and runs entirely after it ("Issue order").
                self._side.wait_stream(main)
                with torch.cuda.stream(self._side):      # (not the capture's origin stream: pass B's decoders never fork there)
                    losses = self._phase_b(ctx)
                    if self.grad_sync is not None and update and not torch.cuda.is_current_stream_capturing():
                        self.grad_sync.start_first()        # bucket 0 is final: its all-reduce runs beside the VAT chain
                vat_loss = self._phase_v(ctx)
                main.wait_stream(self._side)
            else:
                with self._forks(FORK_PASS_A):          # pass B on this (the origin) stream forks as pass A does
                    losses = self._phase_b(ctx)
                vat_loss = self._phase_v(ctx)
        out = {"mix_losses": losses, "vat_loss": vat_loss}
        if self.teacher_w > 0:
            out["teacher_loss"] = ctx["teacher_loss"]
        if self.teacher_T > 0:
            out["teacher_certain"] = ctx["teacher_certain"]
        if self.args["dropout"]:        # (behind _decoder_fork's join: the fp branch never forks its second decoder under capture)
            out["fp_losses"] = self._fp_branch(ctx["uimg_ab"], ctx["pseudo_outputs1"], ctx["pseudo_outputs2"], ctx["inject"], None)
        if self.monitor is not None:    # behind the join of pass B's stream above: both accumulate launches and every loss word are complete
            self._monitor_finalize([l[j:j + 1] for l in losses for j in range(3)] + [vat_loss])
        if update:
            self.exchange_and_update()
        return out

    # ------------------------------------------------------------------ training monitor (chap_amd.monitor; every launch below only with one attached)
    def _monitor_logits(self, logits1, logits2, labels, n_first):
        """Behind pseudo_block, on its stream: the counts of the two heads' arg-max maps against the samples' own labels."""
        ops.monitor_accumulate(logits1, logits2, labels, self.monitor.ws, n_first)

    def _monitor_maps(self, map1, map2, labels, n_first):
        """Behind largest_cc, on pass B's stream: the Dice terms of the filtered maps.  Writes its own region of the workspace."""
        ops.monitor_accumulate_labels(map1, map2, labels, self.monitor.ws, n_first, self.args["num_classes"])

    def _monitor_finalize(self, scalars, has_labels=True):
        m = self.monitor
        ops.monitor_finalize(m.ws, m.ring, self._sched[self._mon_at:self._mon_at + 2], m.C, scalars, has_labels)

    @contextlib.contextmanager
    def _decoder_fork(self, origin):
        """Under capture: the passes on `origin` inside may run their second decoder on a stream forked from it (a captured stream may fork / join
        with the capture's ORIGIN stream only, see __init__); which of them do is decided pass by pass (_forks) against CHAP_FORK_MASK, read here
        once per captured iteration."""
        capturing = self.concurrent and torch.cuda.is_current_stream_capturing()
        if capturing:
            self._d2.wait_stream(origin)
            self._fork_sides, self._fork_mask = {origin.cuda_stream: self._d2}, switch("CHAP_FORK_MASK")
        try:
            yield
        finally:
            if capturing:
                origin.wait_stream(self._d2)
                self._fork_sides = {}

    @contextlib.contextmanager
    def _forks(self, bit=None):
        """Around one pass (a forward or a backward of the model) on the capture's origin stream: inside, the executor forks the pass's second decoder
        if CHAP_FORK_MASK has `bit` (FORK_*; None: regardless of the mask) -- that is, Executor._side_stream answers with _decoder_fork's stream -- and
        groups the two decoders' launches otherwise.  Outside _decoder_fork (eager, single-stream step) it changes nothing."""
        ex = self.model._exec
        old = ex._capture_sides
        ex._capture_sides = self._fork_sides if (bit is None or self._fork_mask & bit) else {}
        try:
            yield
        finally:
            ex._capture_sides = old

    def _phase_a(self, volume_batch, label_batch, inject):
        a, model = self.args, self.model
        inject = inject or {}
        lbs = a["labeled_bs"]
        B = volume_batch.shape[0]
        lsub, usub = lbs // 2, (B - lbs) // 2
        ctx = dict(inject=inject, volume_batch=volume_batch, lsub=lsub, usub=usub,
                   img_a=volume_batch[:lsub], img_b=volume_batch[lsub:lbs], uimg_a=volume_batch[lbs:lbs + usub], uimg_b=volume_batch[lbs + usub:],
                   lab_a=label_batch[:lsub], lab_b=label_batch[lsub:lbs], uimg_ab=volume_batch[lbs:])
        # ---- the first VAT power-iteration forward (x + xi * d) needs nothing from pass A: it runs beside it on its own stream
        main = torch.cuda.current_stream()
        # (`vat_early`, default on since the end of round 2: 2D 7.60 -> 7.41 ms, 3D 18.29 -> 17.75 ms per step.  It had been off because
        #  two identical runs were not always bitwise equal with it; the cause was not this overlap but dropout seeds drawn in ISSUE
        #  order -- see Executor.forward -- together with stream handles repeating in PyTorch's pool, see ChapStep.__init__.)
        pre = self._pre if (self.concurrent and a["adv_noise"] and a.get("vat_early", True)) else None
        model.prepare_weights()                  # before the streams fork: every pass of the iteration reads the same packed copies
        if self.teacher_w > 0:                   # the optimizer launch rewrote the teacher's flat buffer: its packed copies too, here and not on pass B's stream
            self.teacher.set_compute_dtype(model.compute_dtype)
            if torch.cuda.is_current_stream_capturing():
                self.teacher.mark_params_dirty()        # the pack launch is a node of every captured iteration, whatever was packed before the capture
            self.teacher.prepare_weights()
        if a["adv_noise"]:
            if pre is not None:
                # The early pass runs on its own stream beside pass A and is issued in FRONT of it (round 4 tried issuing it between pass A's encoder and
                # its decoders: 6.95 vs 6.5 ms -- it then shares a queue with pass A)
                pre.wait_stream(main)
                with torch.enable_grad(), torch.cuda.stream(pre):
                    ctx["vat_state"] = self.adv_loss.begin(model, volume_batch, B - lbs, inject)
            else:
                with self._forks():                 # the first VAT forward on this (the origin) stream forks whatever the mask says
                    ctx["vat_state"] = self.adv_loss.begin(model, volume_batch, B - lbs, inject)
        # ---- pass A: pseudo labels from both decoders (no grad), train_ours_2D.py:314-330
        with self._forks(FORK_PASS_A), torch.no_grad():
            pre_ab1, pre_ab2 = model(ctx["uimg_ab"], drop_masks=inject.get("drop_A"))
            soft1, soft2, pseudo1, pseudo2, knowledge = ops.pseudo_block(pre_ab1, pre_ab2)
            if self.monitor is not None:        # the unlabelled samples' labels are in every batch (the reference's ulab_a / ulab_b)
                ctx["ulab"] = label_batch[lbs:]
                self._monitor_logits(pre_ab1, pre_ab2, ctx["ulab"], 0)
        if pre is not None:
            main.wait_stream(pre)
        ctx.update(outputs_soft1=soft1, outputs_soft2=soft2, pseudo_outputs1=pseudo1, pseudo_outputs2=pseudo2, knowledge=knowledge)
        # ---- the VAT branch (:368-375) depends only on pass A: it and pass B run side by side on two streams and
        #      accumulate their parameter gradients into separate buckets (VAT: the second one)
        if a["adv_noise"]:
            ctx["diff_mask"] = ops.diff_mask(pseudo1, pseudo2, knowledge, 4, a["topk1"])
        return ctx

    def _phase_b(self, ctx):
        """Largest-CC filter, loss mask and BCP mixing (:326-338) feed pass B only: they run at the head of this branch, off
        the critical path (the VAT branch needs the soft / arg-max outputs, not these); then pass B and the four mix_loss
        terms (:339-351), backward into gradient bucket 0."""
        a, model, inject = self.args, self.model, ctx["inject"]
        nc = a["num_classes"]
        lsub, usub, volume_batch = ctx["lsub"], ctx["usub"], ctx["volume_batch"]
        with torch.no_grad():
            batch = self.passb_batch
            stacked = ops._stacked_pair(ctx["pseudo_outputs1"], ctx["pseudo_outputs2"]) if (batch and a["nms"]) else None
            if stacked is not None:             # the components of an image do not depend on its neighbours in the batch: one call for both heads
                plab = ops.largest_cc(stacked, nc)
                plab1, plab2 = plab[:plab.shape[0] // 2], plab[plab.shape[0] // 2:]
            elif a["nms"]:
                plab1 = ops.largest_cc(ctx["pseudo_outputs1"], nc)
                plab2 = ops.largest_cc(ctx["pseudo_outputs2"], nc)
            else:
                plab1, plab2 = ctx["pseudo_outputs1"], ctx["pseudo_outputs2"]
            if self.monitor is not None:
                self._monitor_maps(plab1, plab2, ctx["ulab"], 0)
            loss_mask = torch.empty(lsub, *volume_batch.shape[2:], dtype=torch.int64, device=volume_batch.device)
            # BCP mixing (:335-338): net_input_mix = cat(net_input_l, net_input_unl)
            net_input_mix = torch.empty((lsub + usub,) + tuple(volume_batch.shape[1:]), dtype=torch.float32, device=volume_batch.device)
            if batch:
                ops.bcp_mix(ctx["img_b"], ctx["uimg_b"], net_input_mix[:lsub], ctx["uimg_a"], ctx["img_a"], net_input_mix[lsub:], loss_mask, self.box)
            else:
                ops.box_mask(loss_mask, self.box)
                ops.box_mix(ctx["img_b"], ctx["uimg_b"], net_input_mix[:lsub], self.box)       # img_b*mask + uimg_b*(1-mask)
                ops.box_mix(ctx["uimg_a"], ctx["img_a"], net_input_mix[lsub:], self.box)       # uimg_a*mask + img_a*(1-mask)
        lab_a, lab_b = ctx["lab_a"], ctx["lab_b"]
        plab_a1, plab_b1 = plab1[:usub], plab1[usub:]
        plab_a2, plab_b2 = plab2[:usub], plab2[usub:]
        out_mix1, out_mix2 = model(net_input_mix, drop_masks=inject.get("drop_B"))
        # the teacher's pass behind the student's (whose dropout seeds are the ones it draws without a teacher), on this stream
        tch = self._teacher_pass(net_input_mix, inject) if self.teacher_w > 0 else None
        # with teacher_uncertainty = T: pass 0 above stays the target, T - 1 more passes follow, each under its own noise draw (and dropout seeds)
        tpasses = [tch] + [self._teacher_pass(net_input_mix, inject, k) for k in range(1, self.teacher_T)] if self.teacher_T > 0 else None
        d1, d2 = torch.empty_like(out_mix1), torch.empty_like(out_mix2)
        terms = (  # (logits, dlogits, img_l, patch_l, unlab)
            (out_mix1[lsub:], d1[lsub:], plab_a2, lab_a, True),      # mix_loss1: out_unl1
            (out_mix2[lsub:], d2[lsub:], plab_a1, lab_a, True),      # mix_loss2: out_unl2
            (out_mix1[:lsub], d1[:lsub], lab_b, plab_b2, False),     # mix_loss3: out_l1
            (out_mix2[:lsub], d2[:lsub], lab_b, plab_b1, False),     # mix_loss4: out_l2
        )
        losses = []
        split = self.gradsim is not None and inject.get("sim_score") is None and self.sim_score is None
        if split:       # loss_l / loss_u (:352-353) are taken apart: e* holds the unlabeled-supervised parts' gradient
            e1, e2 = torch.empty_like(out_mix1), torch.empty_like(out_mix2)
            eterms = (e1[lsub:], e2[lsub:], e1[:lsub], e2[:lsub])
        # the batched loss launch is built for the two benchmarked class counts; every other count issues the four single-term calls
        # below (bit-identical by construction), while largest-CC and the BCP mixing above stay batched: they carry no class limit
        batch = batch and nc in ops.MIX_LOSS_MULTI_CLASSES
        if batch:       # the four terms are independent: one launch per kernel for all of them (with `split`, the dl set and the e set)
            base = [dict(logits=lg, target_a=img_l, target_b=patch_l, mask=loss_mask) for lg, _, img_l, patch_l, _ in terms]
            wts = [(0.5, 1.0) if unlab else (1.0, 0.5) for *_, unlab in terms]                   # l_weight=1.0, u_weight=0.5 (:198-203)
            fwd = ops.mix_loss_multi_fwd([dict(b, w_a=iw, w_b=pw) for b, (iw, pw) in zip(base, wts)])
            losses = [l for l, _ in fwd]
            bwd = lambda ws, outs: ops.mix_loss_multi_bwd([dict(b, w_a=w[0], w_b=w[1], acc=acc, dlogits=o) for b, w, (_, acc), o in zip(base, ws, fwd, outs)])
            if split:
                wl = [(0.0, pw) if unlab else (iw, 0.0) for (iw, pw), (*_, unlab) in zip(wts, terms)]
                wu = [(iw, 0.0) if unlab else (0.0, pw) for (iw, pw), (*_, unlab) in zip(wts, terms)]
                bwd(wl, [t[1] for t in terms])
                bwd(wu, eterms)
            else:
                bwd(wts, [t[1] for t in terms])
        for ti, (lg, dl, img_l, patch_l, unlab) in enumerate(() if batch else terms):
            iw, pw = (0.5, 1.0) if unlab else (1.0, 0.5)            # l_weight=1.0, u_weight=0.5 (:198-203)
            loss3, acc = ops.mix_loss_fwd(lg, img_l, patch_l, loss_mask, iw, pw)
            if split:   # (loss_image, loss_patch) = (loss_u_out, loss_l_in) for the unlabeled rows, (loss_l_out, loss_u_in) for the labeled ones (:345-349)
                wl, wu = ((0.0, pw), (iw, 0.0)) if unlab else ((iw, 0.0), (0.0, pw))
                ops.mix_loss_bwd(lg, img_l, patch_l, loss_mask, wl[0], wl[1], acc, dl)
                ops.mix_loss_bwd(lg, img_l, patch_l, loss_mask, wu[0], wu[1], acc, eterms[ti])
            else:
                ops.mix_loss_bwd(lg, img_l, patch_l, loss_mask, iw, pw, acc, dl)
            losses.append(loss3)
        if tch is not None:
            # softmax-MSE of both heads against the teacher's ensemble, weighted cw * teacher_consistency; its gradient is added to what mix_loss_bwd
            # has just written -- with `split` to the e set: the term is unsupervised (loss_u) -- and the backward below carries it
            ctx["teacher_loss"] = torch.empty(1, dtype=torch.float32, device=out_mix1.device)
            if tpasses is None:
                ops.teacher_consistency((out_mix1, out_mix2), tch, ctx["teacher_loss"], (e1, e2) if split else (d1, d2), gscale=self.teacher_w,
                                        gscale_dev=self.cw_dev, accumulate=True)
            else:
                # the term only where the entropy of the T passes' mean prediction lies under the scheduled threshold, normalised by the count
                # of such pixels (this rank's own): a masked-out pixel's gradient stays what mix_loss_bwd wrote
                certain, count = ops.teacher_uncertainty(tpasses, threshold_dev=self.thr_dev)
                ctx["teacher_certain"] = count
                self.teacher_pixels = certain.numel()       # N * P of the term: count / teacher_pixels is the certain share
                ops.teacher_consistency_masked((out_mix1, out_mix2), tch, certain, count, ctx["teacher_loss"], (e1, e2) if split else (d1, d2),
                                               gscale=self.teacher_w, gscale_dev=self.cw_dev, accumulate=True)
        if not split:
            torch.autograd.backward([out_mix1, out_mix2], [d1, d2])
            return losses
        # two backward passes over the saved forward (linear in dlogits): gradients of loss_l and of loss_u into their own
        # buffers -> the channel scores of the NEXT iteration (gradsim.get_grad_convkernel, :365); their sum is the BCP
        # gradient the single pass would have produced
        n_ = self._grad_lu.numel() // 2
        g_l, g_u = self._grad_lu[:n_], self._grad_lu[n_:]
        self._grad_lu.zero_()
        model.backward_saved(out_mix1, [d1, d2], g_l)
        model.backward_saved(out_mix1, [e1, e2], g_u)
        model.release_saved(out_mix1)
        self._new_scores_from = (g_l, g_u)
        b0 = self.grad_both[:n_]
        ops.perturb(b0, g_l, b0, 1.0)
        ops.perturb(b0, g_u, b0, 1.0)
        return losses

    def _teacher_pass(self, x, inject, k=0):
        """The mean teacher's prediction on x + u, u uniform in [-teacher_noise, teacher_noise) (Tarvainen and Valpola; the public code adds a clipped
        Gaussian, DESIGN.md "Mean teacher"), on the current stream and without gradients: nothing is saved.  BatchNorm normalises with the batch's
        own statistics (the public code never puts its ema_model into eval()) and updates no running buffer; the shift of the statistics' sums is
        the iteration's snapshot of the STUDENT's running means, so the teacher's own never-updated ones play no role.  The noise seed and the
        seeds of the dropout sites come from the student's generator, in program order: one stream, one checkpointed state.  `k`: which of the
        teacher_uncertainty passes this is (0: the target's, the only one of the plain term); every pass draws its own noise."""
        model, t = self.model, self.teacher
        noise = float(self.args["teacher_noise"])
        with torch.no_grad():
            x_t = x
            if noise > 0:
                u = inject.get("teacher_u")             # (tests: a static noise tensor, as `d0` is the VAT branch's; a list: one per pass)
                if isinstance(u, (list, tuple)):
                    u = u[k]
                if u is None:
                    u = torch.empty_like(x)
                    ops.rand_uniform(u, model._rng.next_seed(), -noise, noise, seed_dev=model._rng.seed_dev)
                x_t = torch.empty_like(x)
                ops.perturb(x, u, x_t, 1.0)
            t._ensure_flat()
            old = (t._rng, t._shift_hold, t.training)
            t._rng, t._shift_hold, t.training = model._rng, model._shift_hold, True
            try:
                t1, t2 = t(x_t, update_stats=False, drop_masks=inject.get("drop_T"))
            finally:
                t._rng, t._shift_hold, t.training = old
        return t1, t2

    def _phase_v(self, ctx):
        a = self.args
        if not a["adv_noise"]:
            return torch.zeros(1, dtype=torch.float32, device=ctx["volume_batch"].device)
        return self.adv_loss.finish(self.model, ctx["vat_state"], ctx["outputs_soft1"], ctx["outputs_soft2"], ctx["diff_mask"], a["adv_losstype"],
                                    weight_dev=self.cw_dev, grad_buffer=self.grad2, forks=self._forks)

    def _fp_branch(self, uimg_ab, pseudo1, pseudo2, inject, capturing):
        """"2) fp" of the loop (train_ours_2D.py:359-365, default off): both decoders on the channel-perturbed features
        (DualDecoder.forward(dropout=True)), cross-entropy against the other head's pseudo labels, weighted with the
        consistency weight like the VAT term (:378).  Upstream compares the 1.5 U logits with U labels (a shape error) and
        reads the scores from the absent grad.GradSim: here every output row is paired with its own sample's pseudo label,
        cat(pseudo, pseudo[U/2:]), and the scores are `self.sim_score`.  Runs after the VAT branch on the main stream
        and accumulates into the second gradient bucket; the consistency weight is read from device memory (`cw_dev`), so
        the branch is part of a captured iteration like everything else."""
        a, model = self.args, self.model
        if self.dims != 2:
            raise NotImplementedError("chap_amd: the dropout (fp_loss) branch exists for the 2D DualDecoder only, as upstream")
        U = uimg_ab.shape[0]
        scores = inject.get("sim_score", self.sim_score)
        produced = scores is None and self.gradsim is not None
        if produced:
            scores = self.gradsim.get_sim()                     # of the previous iteration (:360)
        o1, o2 = model(uimg_ab, False, True, [0, 1, 2, 3, 4], scores, a["comp_drop"],
                       drop_masks=inject.get("drop_FP"), drop_uniforms=inject.get("fp_uniforms"),
                       drop_branches=inject.get("fp_branches"), grad_buffer=self.grad2)
        t1, t2 = torch.cat((pseudo1, pseudo1[U // 2:])), torch.cat((pseudo2, pseudo2[U // 2:]))
        losses, ds = [], []
        for o, t in ((o1, t2), (o2, t1)):
            l3, acc = ops.mix_loss_fwd(o, t, None, None, 1.0, 0.0, k_dice=0.0, k_ce=1.0)        # mean cross-entropy
            d = torch.empty_like(o)
            ops.mix_loss_bwd(o, t, None, None, 1.0, 0.0, acc, d, gscale_dev=self.cw_dev, k_dice=0.0, k_ce=1.0)
            losses.append(l3[0:1])
            ds.append(d)
        torch.autograd.backward([o1, o2], ds)
        if produced:                                            # :365, after the perturbed pass has read the old scores
            self.gradsim.get_grad_convkernel(self._new_scores_from[0], self._new_scores_from[1], model, self.opt, self.iter_num)
        return losses

    def step(self, volume_batch, label_batch, box_yx=None, inject=None):
        self._hw = tuple(volume_batch.shape[2:])
        self.prepare(box_yx)
        out = self.device_step(volume_batch, label_batch, inject)
        self.finish()
        return out

    # ------------------------------------------------------------------ HIP graph capture
    def capture(self, volume_batch, label_batch, warmup=3, inject=None, restore=True):
        """Capture device_step() into one HIP graph over static input buffers; afterwards call
        replay(volume_batch, label_batch).  The `warmup` eager iterations (allocator, packed-weight tables, lazily set
        kernel attributes: nothing of that may happen for the first time under capture) run on the given batch; with
        `restore` (default) parameters, momentum, BatchNorm statistics, iter_num / LR and the RNG state are put back
        afterwards, so capture() does not train -- without it they count as `warmup` real iterations.  The captured pass
        itself is not executed: iter_num == number of applied updates at all times.  `inject` (tests): static tensors
        (dropout masks, VAT noise) the captured iteration reads instead of drawing its own."""
        check_graph_environment(self.concurrent)
        self._hw = tuple(volume_batch.shape[2:])
        self._static_v = volume_batch.clone()
        self._static_l = label_batch.clone()
        snap = self.state_dict() if (restore and warmup > 0) else None
        mon_snap = self.monitor.snapshot() if (snap is not None and self.monitor is not None) else None
        guard_snap = self.guard.snapshot() if (snap is not None and self.guard is not None) else None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self.prepare()
                self.device_step(self._static_v, self._static_l, inject)
                self.finish()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if snap is not None:
            self.load_state_dict(snap)
            if mon_snap is not None:            # the warm-up iterations' rows go with their updates
                self.monitor.restore(mon_snap)
            if guard_snap is not None:          # ... and so do the guard's rows and counts
                self.guard.restore(guard_snap)
            torch.cuda.synchronize()
        self.model._rng.reset_counter()
        np_state = np.random.get_state()
        self.prepare()                          # the schedule block must hold valid values while the graph is being captured ...
        if restore:
            np.random.set_state(np_state)       # ... but its BCP-box draw is not an iteration's: capture() leaves the numpy stream untouched
        # the four-graph form only when bucket 0 is to be all-reduced beside the VAT chain; the fold schedule exchanges once, at the
        # end: [compute graph] -> all-reduce -> [optimizer graph] keeps pass B and the VAT chain as forked branches of ONE graph
        if (self.grad_sync is not None and getattr(self.grad_sync, "overlap", False) and type(self)._iteration is ChapStep._iteration
                and self.concurrent and self.args["adv_noise"]):
            return self._capture_dp(inject)
        g = torch.cuda.CUDAGraph()
        dp = self.grad_sync is not None
        # thread_local: the RCCL watchdog thread polls events while we capture (global mode would abort on that)
        with torch.cuda.graph(g, stream=self._cap, capture_error_mode="thread_local"):
            self.model._rng.seed_dev.add_(1)
            self._static_out = self.device_step(self._static_v, self._static_l, inject, update=not dp)
        self._graph, self._graph_opt, self._graphs_dp = g, None, None
        if dp:          # data-parallel without the two-branch schedule: [compute graph] -> RCCL all-reduce (eager) -> [optimizer graph]
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, pool=g.pool(), stream=self._cap, capture_error_mode="thread_local"):
                self.opt.step(grad_scale=1.0 / self.world_size, grad2=self.grad2)
            self._graph_opt = g2
        return g

    def _capture_dp(self, inject):
        """Data-parallel capture: the iteration as FOUR graphs so that RCCL (never captured) can run between them and the
        all-reduce of bucket 0 overlaps the VAT chain (north_star):

            main:  [A: pass A, pseudo labels, mask] -> [V: VAT chain -> bucket 1] -> all-reduce(bucket 1) ----+-> [optimizer]
            side:                       wait A -> [B: LCC, BCP mix, pass B -> bucket 0] -> all-reduce(bucket 0) --^

        B and V are captured into SEPARATE memory pools (they run concurrently at replay: sharing a pool would let one
        reuse memory the other has freed during capture); what crosses graph boundaries (pass A's outputs) is kept alive
        by `self._dp_ctx`.  Each capture's origin stream forks its own second-decoder stream."""
        kw = dict(capture_error_mode="thread_local", stream=self._cap)
        stack = contextlib.ExitStack()
        gA, gB, gV, gO = (torch.cuda.CUDAGraph() for _ in range(4))
        with torch.cuda.graph(gA, **kw):
            self.model._rng.seed_dev.add_(1)
            stack.enter_context(self.model.hold_stat_shift())       # the snapshot copy is a node of graph A; held until V is captured
            with self._decoder_fork(torch.cuda.current_stream()):
                ctx = self._phase_a(self._static_v, self._static_l, inject)
        with torch.cuda.graph(gB, **kw):
            with self._decoder_fork(torch.cuda.current_stream()), self._forks():      # graph B's pass B forks whatever the mask says
                losses = self._phase_b(ctx)
        with torch.cuda.graph(gV, **kw):
            with self._decoder_fork(torch.cuda.current_stream()):
                vat_loss = self._phase_v(ctx)
            out = {"mix_losses": losses, "vat_loss": vat_loss}
            if self.teacher_w > 0:
                out["teacher_loss"] = ctx["teacher_loss"]
            if self.teacher_T > 0:
                out["teacher_certain"] = ctx["teacher_certain"]
            if self.args["dropout"]:    # (behind _decoder_fork's join, as in _iteration: no fork)
                out["fp_losses"] = self._fp_branch(ctx["uimg_ab"], ctx["pseudo_outputs1"], ctx["pseudo_outputs2"], ctx["inject"], None)
        stack.close()
        with torch.cuda.graph(gO, **kw):
            if self.monitor is not None:        # graphs B and V have both run when this one is replayed
                self._monitor_finalize([l[j:j + 1] for l in losses for j in range(3)] + [vat_loss])
            self.opt.step(grad_scale=1.0 / self.world_size, grad2=self.grad2)
        self._dp_ctx, self._static_out = ctx, out
        self._graph, self._graph_opt, self._graphs_dp = None, None, (gA, gB, gV, gO)
        return gA

    def _stage(self, fill):
        """fill(image_out, label_out) on the copy stream, into the staging buffers, behind the hand-over of the batch staged before."""
        if self._stage_v is None:
            self._stage_v, self._stage_l = torch.empty_like(self._static_v), torch.empty_like(self._static_l)
            self._copy_stream = torch.cuda.Stream(device=self._static_v.device)
            self._staged_evt, self._taken_evt = torch.cuda.Event(), None
        with torch.cuda.stream(self._copy_stream):
            if self._taken_evt is not None:
                self._copy_stream.wait_event(self._taken_evt)      # the previous staged batch has been moved into the static buffers
            fill(self._stage_v, self._stage_l)
            self._staged_evt.record(self._copy_stream)
        self._staged = True

    def stage(self, volume_batch, label_batch):
        """Start the host-to-device copy of the NEXT batch on a copy stream, beside the iteration that is running: the loader of
        train_ours_2D.py:301-304 yields CPU tensors and `.cuda()`s them on the compute stream (19 MB per 2D iteration, 0.4 ms of PCIe time in front
        of every step; 3D 1.0 ms).  replay() without a batch then takes the staged one (a device-to-device copy of microseconds).  Pinned source
        tensors make the copy asynchronous to the host as well."""
        def fill(image_out, label_out):
            image_out.copy_(volume_batch, non_blocking=True)
            label_out.copy_(label_batch, non_blocking=True)
        self._stage(fill)

    def stage_from(self, loader):
        """stage() for a device-resident loader (chap_amd.data.DeviceLoader): instead of a host-to-device copy, the copy stream runs the
        loader's augmentation kernel straight into the staging buffers -- `loader.next_into(image_out, label_out)` launches on the current
        stream -- so the batch of iteration n + 1 is built beside iteration n and replay() takes it as it takes any staged batch."""
        self._stage(loader.next_into)

    def replay(self, volume_batch=None, label_batch=None, box_yx=None):
        if volume_batch is None:
            if not self._staged:
                raise RuntimeError("chap_amd: replay() without a batch needs a stage()d one")
            main = torch.cuda.current_stream()
            main.wait_event(self._staged_evt)
            self._static_v.copy_(self._stage_v, non_blocking=True)
            self._static_l.copy_(self._stage_l, non_blocking=True)
            self._taken_evt = torch.cuda.Event()
            self._taken_evt.record(main)
            self._staged = False
        else:
            self._static_v.copy_(volume_batch, non_blocking=True)
            self._static_l.copy_(label_batch, non_blocking=True)
        self.prepare(box_yx)
        if self._graphs_dp is not None:
            gA, gB, gV, gO = self._graphs_dp
            main = torch.cuda.current_stream()
            gA.replay()
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                gB.replay()
                self.grad_sync.start_first()        # all-reduce of bucket 0 on the side stream, beside graph V
            gV.replay()
            self.grad_sync.start()
            main.wait_stream(self._side)
            self.grad_sync.wait()
            gO.replay()
        else:
            self._graph.replay()
            if self._graph_opt is not None:
                self.grad_sync.start()
                self.grad_sync.wait()
                self._graph_opt.replay()
        # the optimizer inside the graph changed the weights on the device: the packed copies an EAGER forward
        # (validation, inference, step()) would otherwise reuse are stale -- the graph itself re-packs on every replay
        self.model.mark_params_dirty()
        if self.teacher is not None:
            self.teacher.mark_params_dirty()
        self.finish()
        return self._static_out


class AblationStep(ChapStep):
    """One iteration of the ablation loop (train_ablation_2D.py:159-246): ONE full-batch forward, supervised
    0.5*(CE + Dice) of both heads on the labeled half (:171-176), cross pseudo supervision -- CE of each head against
    the other head's arg-max -- on the unlabeled half (:203-207,216-217), the same create_maskV1 + VAT2d pair as the main
    loop (:228-230) and  loss = model1_loss + model2_loss + cw * (w_adv * vat_loss + w_drop * fp_loss)  (:236), then
    SGD + poly LR.  `losses.DiceLoss` is absent upstream: the SSL4MIS definition (1 - (2 sum p t + s)/(sum p^2 + sum t +
    s), s = 1e-5, mean over classes) is used.  The shipped VAT call passes the full-batch soft outputs next to an
    unlabeled-half mask (shape-inconsistent); here, as in the main loop, VAT acts on the unlabeled half.  fp_loss (the
    `dropout` branch, :209-213) is 0 as upstream.  The consistency weight lives in device memory: capture()/replay() work.
    With a monitor: the full-batch forward is scored with n_first = labeled_bs, acc_conf_analysis's split (train_ours_2D.py:157-158)."""

    MONITOR_LAYOUT = "ablation"

    def __init__(self, model, args=None, *pos, **kw):
        if float((args or {}).get("teacher_consistency", 0.0)) > 0:
            raise ValueError("chap_amd AblationStep: teacher_consistency=%g: the mean teacher's consistency term exists in ChapStep's pass B only" % float(args["teacher_consistency"]))
        if (args or {}).get("teacher_uncertainty", 0):
            raise ValueError("chap_amd AblationStep: teacher_uncertainty=%r: the mean teacher's consistency term exists in ChapStep's pass B only" % (args["teacher_uncertainty"],))
        super().__init__(model, args, *pos, **kw)

    def _iteration(self, volume_batch, label_batch, inject=None, update=True):
        a, model = self.args, self.model
        inject = inject or {}
        lbs = a["labeled_bs"]
        out1, out2 = model(volume_batch, drop_masks=inject.get("drop_F"))
        with torch.no_grad():
            soft1, soft2, arg1, arg2, knowledge = ops.pseudo_block(out1[lbs:].contiguous(), out2[lbs:].contiguous())
            if self.monitor is not None:
                self._monitor_logits(out1, out2, label_batch, lbs)
        d1, d2 = torch.empty_like(out1), torch.empty_like(out2)
        lab = label_batch[:lbs].contiguous()
        sup, cps = [], []
        for o, d, other in ((out1, d1, arg2), (out2, d2, arg1)):
            ol, ou = o[:lbs].contiguous(), o[lbs:].contiguous()
            dl, du = torch.empty_like(ol), torch.empty_like(ou)
            l3, acc = ops.mix_loss_fwd(ol, lab, None, None, 1.0, 0.0, smooth=1e-5)            # 0.5*(CE + Dice)
            ops.mix_loss_bwd(ol, lab, None, None, 1.0, 0.0, acc, dl, smooth=1e-5)
            c3, acc2 = ops.mix_loss_fwd(ou, other, None, None, 1.0, 0.0, k_dice=0.0, k_ce=1.0)  # mean CE vs the other head
            ops.mix_loss_bwd(ou, other, None, None, 1.0, 0.0, acc2, du, gscale_dev=self.cw_dev, k_dice=0.0, k_ce=1.0)
            d[:lbs].copy_(dl); d[lbs:].copy_(du)
            sup.append(l3[0:1]); cps.append(c3[0:1])
        torch.autograd.backward([out1, out2], [d1, d2])
        vat_loss = torch.zeros(1, dtype=torch.float32, device=volume_batch.device)
        if a["adv_noise"]:
            diff_mask = ops.diff_mask(arg1, arg2, knowledge, 4, a["topk1"])
            vat_loss = self.adv_loss(model, volume_batch, soft1, soft2, diff_mask, a["adv_losstype"], weight_dev=self.cw_dev,
                                     inject=inject, grad_buffer=self.grad2, weight=a.get("w_adv", 1.0))
        if self.monitor is not None:
            self._monitor_finalize(sup + cps + [vat_loss], has_labels=False)
        if update:
            self.exchange_and_update()
        return {"sup_losses": sup, "cps_losses": cps, "vat_loss": vat_loss, "consistency_weight": self._cw_host}

    def prepare(self, box_yx=None):
        self._cw_host = get_current_consistency_weight(self.iter_num // 150, self.args)      # no BCP box in this loop
        self._upload_sched([], self._cw_host)

    def replay(self, volume_batch=None, label_batch=None, box_yx=None):
        out = super().replay(volume_batch, label_batch, box_yx)
        out["consistency_weight"] = self._cw_host        # the one host-side entry of the (static) output dict
        return out
