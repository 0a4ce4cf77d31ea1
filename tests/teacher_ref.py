"""fp64 restatement of chap_teacher_consistency (include/chap_hip_teacher.h) with a per-element error bound, an fp32 emulation of the kernel's
arithmetic, and the inputs the CPU and GPU tests share (a helper module, not a conftest).

    q = 0.5 (softmax(t1) + softmax(t2)),  p_h = softmax(s_h),  e_h = p_h - q
    loss = sum_h 1/(N C P) sum e_h^2,     g_h,k = G p_k (e_k - sum_c p_c e_c),  G = gscale * gscale_dev * 2 / (N C P)

The bound, in the manner of tests/kernel_ref.py (U32 = 2^-24, gamma(n) for an n-term fp32 chain) and fixed before the first GPU run of the
kernel -- nothing below was fitted to what the kernel gives:
  softmax      e_p = (ew(C) + |z - m| U32) p with ew(C) = max(8, C + 4) U32, the softmax chain of tests/class_count_cases.py
  q            d_q = 0.5 (e_p(t1) + e_p(t2)) + U32 q                  (the add; the halving is exact)
  e            d_e = e_p + d_q + U32 |e|
  loss         per head sum (2 |e| d_e + d_e^2 + U32 e^2) + (gamma(N C P) + U32) sum e^2: the square, the thread / wave / block chain of at most
               N C P terms; the rows are summed in fp64.  The two totals stored as fp32, their sum, fl(N P) fl(C), its reciprocal and the
               product: 6 U32 |loss|
  dot          d_dot = sum_c (e_p,c |e_c| + p_c d_e,c) + (C + 1) U32 sum_c |p_c e_c|      (C products, C - 1 adds, each relative to the partial sums)
  g            |G| (e_p,k |e_k - dot| + p_k (d_e,k + d_dot + U32 |e_k - dot|)) + 6 U32 |g|     (G: two products, fl(N P) fl(C), the division; the two
               products of G p (e - dot))
  accumulate   + U32 |prior + g|: the one rounding of prior + g
Every term is relative to a quantity of the element itself: there is no absolute floor in any comparison."""
import torch

from tests import kernel_ref as kr

CLASSES = tuple(range(2, 9))
SCALAR = (4, (17, 19))              # P = 323, not a multiple of 4: the one-pixel path; two blocks, a ragged last wave
QUADS = (4, (16, 20))               # P = 320 on 16-byte-aligned tensors: the four-pixel path
TWO_TRIPS = (3, (420, 420))         # 529 200 pixels = 132 300 quads > 512 * 256: a second grid-stride trip
TWO_TRIPS_CLASSES = (2, 8)


def ew(C):
    return max(8, C + 4) * kr.U32


def inputs(C, shape, seed=0):
    """Student and teacher logits of one case: 10 randn clamped to +-30 (the max-subtraction matters), with planted +-30 extremes, exact ties of
    the largest logit, and a run of pixels where teacher and student agree exactly (e = 0 up to the heads' average)."""
    N, sp = shape
    g = torch.Generator().manual_seed(4000 + 16 * seed + C)
    mk = lambda: (10 * torch.randn(N, C, *sp, generator=g)).clamp_(-30, 30)
    s1, s2, t1, t2 = mk(), mk(), mk(), mk()
    P = s1[0, 0].numel()
    for k, t in enumerate((s1, s2, t1, t2)):
        flat = t.reshape(N, C, P)
        flat[k % N, 0, (5 + 3 * k)::37] = 30.0
        flat[k % N, C - 1, (5 + 3 * k)::37] = -30.0
        flat[(k + 1) % N, 0, (11 + k)::41] = flat[(k + 1) % N, C - 1, (11 + k)::41]        # ties
    s1.reshape(N, C, P)[0, :, 2::29] = t1.reshape(N, C, P)[0, :, 2::29]
    t2.reshape(N, C, P)[0, :, 2::29] = t1.reshape(N, C, P)[0, :, 2::29]
    return dict(N=N, C=C, sp=sp, s=(s1, s2), t=(t1, t2))


def _softmax(z, C):
    z = z.double()
    m = z.amax(1, keepdim=True)
    ex = torch.exp(z - m)
    p = ex / ex.sum(1, keepdim=True)
    return p, (ew(C) + (z - m).abs() * kr.U32) * p


def teacher_ref(logits, teacher, gscale=1.0, gscale_dev=None, prior=(None, None)):
    """-> dict(loss [1], loss_b [1], g [2], g_b [2], head [2]) in fp64.  g includes `prior` where one is given (the accumulate form), and its
    bound the rounding of that sum.  `head`: the two heads' own means (their sum is the loss)."""
    U = kr.U32
    N, C = logits[0].shape[:2]
    count = logits[0].numel()
    G = kr._fp32_scalar(gscale) * (1.0 if gscale_dev is None else float(gscale_dev)) * 2.0 / count
    (p1, b1), (p2, b2) = _softmax(teacher[0], C), _softmax(teacher[1], C)
    q = 0.5 * (p1 + p2)
    d_q = 0.5 * (b1 + b2) + U * q
    loss, loss_b, gs, gbs, heads = 0.0, 0.0, [], [], []
    for h in range(2):
        p, e_p = _softmax(logits[h], C)
        e = p - q
        d_e = e_p + d_q + U * e.abs()
        sq = (e * e).sum()
        heads.append(sq / count)
        loss = loss + sq / count
        loss_b = loss_b + ((2 * e.abs() * d_e + d_e * d_e + U * e * e).sum() + (kr.gamma(count) + U) * sq) / count
        dot = (p * e).sum(1, keepdim=True)
        d_dot = (e_p * e.abs() + p * d_e).sum(1, keepdim=True) + (C + 1) * U * (p * e).abs().sum(1, keepdim=True)
        r = e - dot
        g = G * p * r
        g_b = abs(G) * (e_p * r.abs() + p * (d_e + d_dot + U * r.abs())) + 6 * U * g.abs()
        if prior[h] is not None:
            g = prior[h].double() + g
            g_b = g_b + U * g.abs()
        gs.append(g)
        gbs.append(g_b)
    loss_b = loss_b + 6 * U * abs(float(loss))
    as1 = lambda v: torch.as_tensor(float(v), dtype=torch.float64).reshape(1)
    return dict(loss=as1(loss), loss_b=as1(loss_b), g=gs, g_b=gbs, head=[as1(v) for v in heads])


FAULTS = ("no_dot", "div_np", "one_head", "no_two")


def emulate_f32(logits, teacher, gscale=1.0, gscale_dev=None, prior=(None, None), fault=None):
    """The kernel's arithmetic in fp32 torch ops (the same operations in the same order; torch's exp in place of expf, its sum in place of the
    kernel's reduction) -> (loss [1] fp32, [g1, g2] fp32).  `fault` plants one of FAULTS:
      no_dot    the sum_c p_c e_c term of the gradient dropped       div_np   1 / (N P) where 1 / (N C P) belongs (loss and gradient)
      one_head  the target taken from the teacher's first head        no_two   the factor 2 of the gradient missing"""
    f = torch.float32
    N, C = logits[0].shape[:2]
    count = logits[0].numel()
    div = count // C if fault == "div_np" else count

    def sm(z):
        z = z.to(f)
        ex = torch.exp(z - z.amax(1, keepdim=True))
        return ex * (1.0 / ex.sum(1, keepdim=True))

    q = sm(teacher[0]) if fault == "one_head" else 0.5 * (sm(teacher[0]) + sm(teacher[1]))
    two = 1.0 if fault == "no_two" else 2.0
    gs = torch.tensor(gscale, dtype=f) * (torch.tensor(1.0 if gscale_dev is None else float(gscale_dev), dtype=f)) * (torch.tensor(two, dtype=f) / torch.tensor(float(div), dtype=f))
    tot, out = torch.zeros((), dtype=torch.float64), []
    for h in range(2):
        p = sm(logits[h])
        e = p - q
        tot = tot + (e * e).sum(dtype=torch.float64).float().double()
        dot = torch.zeros_like(e[:, :1]) if fault == "no_dot" else (p * e).sum(1, keepdim=True)
        g = gs * p * (e - dot)
        out.append(g if prior[h] is None else prior[h].to(f) + g)
    loss = (tot.float() * (torch.tensor(1.0, dtype=f) / torch.tensor(float(div), dtype=f))).reshape(1)
    return loss, out
