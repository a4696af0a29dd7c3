"""Inputs and float64 recompositions shared by the atom-vocabulary tests (tests/test_vocab_cpu.py, tests/test_gpu_vocab.py):
class counts other than the 15 of `add_aromatic` -- 10 (`basic`), 23 (`full`, the sampling script's fall-back) and the boundaries
of the kernels the class count selects (2, 16 | 17, 32)."""
import numpy as np
import torch

import precision as P
from util import O, synth

POSTERIOR_CLASSES = (2, 10, 15, 16, 17, 23, 32)
POSTERIOR_COUNTS = np.array([27, 26, 25, 24, 20, 9], np.int64)      # N = 131: no multiple of 16 or 128
POSTERIOR_SEED = 77
POSTERIOR_STEPS = 3                                                  # t = 2, 1, 0: the last step has sig = 0 and tm1 clamped
RAGGED_COUNTS = np.array([1, 2, 9, 17, 30], np.int64)                # N = 59


def all_classes(n, C, tag, seed):
    """(n,) int64 atom types holding every class 0..C-1 (n >= C), in hashed order."""
    assert n >= C
    return ((np.arange(n) % C)[np.argsort(synth.hash_u24(n, tag, seed), kind="stable")]).astype(np.int64)


def counts_batch(counts, C, seed, steps=0):
    """A batch of the given molecule sizes with every class among its atom types; with steps > 0 also the hash noise."""
    counts = np.asarray(counts, np.int64)
    n, b = int(counts.sum()), len(counts)
    bb = dict(counts=counts, batch=np.repeat(np.arange(b, dtype=np.int64), counts), init_pos=synth.hash_normal((n, 3), 101, seed),
              init_v=all_classes(n, C, 102, seed), shape=synth.hash_normal((b, 32, 3), 103, seed))
    if steps:
        eps, u = zip(*[synth.step_noise(n, C, s, seed=seed) for s in range(steps)])
        bb["eps"], bb["u"] = np.stack(eps), np.stack(u)
    return bb


def ragged_timesteps():
    return np.array([0, 999, 400, 77, 500], np.int64)


# ------------------------------------------------------------------------------------------------------------------------
# one reverse step in float64 (oracle.posterior_step, every operation in double; the schedule tables, the predictions, the
# state and the noise are the float32 inputs)
# ------------------------------------------------------------------------------------------------------------------------
def _lae(a, b):
    m = torch.max(a, b)
    return m + torch.log(torch.exp(a - m) + torch.exp(b - m))


def posterior_step64(sd, C, pos, v, pred_pos, pred_v, batch, t, eps, u):
    """dict(x, v0, vt, score) float64 arrays of one reverse step."""
    d = lambda a: torch.as_tensor(a).double()      # noqa: E731
    tb = t[batch]
    tab = lambda k, idx: sd[k].double()[idx].unsqueeze(-1)      # noqa: E731
    nonzero = (t != 0).double()[batch].unsqueeze(-1)
    x = (tab("posterior_mean_c0_coef", tb) * d(pred_pos) + tab("posterior_mean_ct_coef", tb) * d(pos)) \
        + nonzero * (0.5 * tab("posterior_logvar", tb)).exp() * d(eps)
    v0 = torch.log_softmax(d(pred_v), dim=-1)
    lvt = torch.log(torch.nn.functional.one_hot(torch.as_tensor(v), C).double().clamp(min=1e-30))
    tm1 = torch.where(t - 1 < 0, torch.zeros_like(t), t - 1)[batch]
    logc = float(np.log(float(C)))
    a = _lae(v0 + tab("log_alphas_cumprod_v", tm1), tab("log_one_minus_alphas_cumprod_v", tm1) - logc)
    b = _lae(lvt + tab("log_alphas_v", tb), tab("log_one_minus_alphas_v", tb) - logc)
    un = a + b
    vt = un - torch.logsumexp(un, dim=-1, keepdim=True)
    score = -torch.log(-torch.log(d(u) + 1e-30) + 1e-30) + vt
    return {k: val.numpy() for k, val in (("x", x), ("v0", v0), ("vt", vt), ("score", score))}


def posterior_step32(sd, dm, pos, v, pred_pos, pred_v, batch, t, eps, u):
    """The same outputs from oracle.posterior_step itself (float32), plus the types it samples."""
    T = lambda a: torch.as_tensor(a)      # noqa: E731
    x, vn, v0, vt = O.posterior_step(sd, dm, T(pos), T(v), T(pred_pos), T(pred_v), batch, t, T(eps), T(u))
    score = -torch.log(-torch.log(T(u) + 1e-30) + 1e-30) + vt
    return {"x": x.numpy(), "v0": v0.numpy(), "vt": vt.numpy(), "score": score.numpy(), "v": vn.numpy()}


def step_gate(got, r32, r64):
    """The repository's gate (precision.bound) on one step's outputs, and the check of the sampled types.

    got: dict(x, v0, vt, v) of the implementation under test.  Returns ({output: (e, e32, e / bound(e32))}, wrong, excluded):
    `wrong` = atoms whose sampled type is not the float64 arg-max although its top-two score gap exceeds 2 * bound(e32 of the
    score) * max|score64| (each of the two scores may be off by the bound), `excluded` = atoms with a smaller gap."""
    g = {}
    for k in ("x", "v0", "vt"):
        e, e32 = P.rel_err(got[k], r64[k]), P.rel_err(r32[k], r64[k])
        g[k] = (e, e32, e / P.bound(e32))
    s = r64["score"]
    top = np.sort(s, -1)
    thr = 2.0 * P.bound(P.rel_err(r32["score"], s)) * float(np.abs(s).max())
    clear = (top[:, -1] - top[:, -2]) > thr
    wrong = int((clear & (np.asarray(got["v"]) != s.argmax(-1))).sum())
    return g, wrong, int((~clear).sum())
