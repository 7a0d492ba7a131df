"""What umlh_seq_step_stats computes (include/umlh.h, ABI v11), stated in numpy float64, and the reference's own expressions
(MultiBench/train.py:403-426) evaluated in fp32 in the reference's order.

``step_stats`` is the contract: with len_b = clamp(lengths[b], 0, T) and sums over b, 0 <= t < T - 1 and the d columns,

    trivial = sum [t < len_b]     (x[b,t,c]     - x[b,t+1,c])^2 / (d #{(b,t): t < len_b}     + 1e-8)      mask[:, :-1]
    recon   = sum [t + 1 < len_b] (recon[b,t,c] - x[b,t+1,c])^2 / (d #{(b,t): t + 1 < len_b} + 1e-8)      mask[:, 1:]

Pairs a predicate excludes are left out of the sums, so Inf or NaN in them does not matter.  Its three keyword switches turn
it into the deliberately wrong restatements tests/test_stepstats_cpu.py must be able to tell apart.

``BOUND``: tests/golden/step_stats.npz records what the reference's own train() logged on the CPU (fp32 torch) for the tensors
it stores; the largest relative difference between those logged values and ``step_stats`` on the same tensors was 1.33e-07,
measured by scripts/make_golden_stepstats.py; 8 x that, rounded up to a power of two, is 2^-19 = 1.91e-06, stored in the file as
``bound`` and repeated here."""
import numpy as np

BOUND = 2.0 ** -19
# the columns of the fixture's "<run>::logged" arrays [step, key]: what the reference handed to wandb.log at each step
LOGGED_KEYS = ("train/loss_x", "train/loss_y", "train/loss", "train/recon_y_loss", "train/loss_x_norm", "train/loss_y_norm",
               "train/loss_private", "train/trivial_loss_x", "train/trivial_loss_y", "train/diff_next_x", "train/diff_next_y")


def clamp_lengths(lengths, B, T):
    if lengths is None:
        return np.full(B, T, dtype=np.int64)
    return np.clip(np.asarray(lengths, dtype=np.int64).reshape(-1), 0, T)


def step_stats(x, lengths=None, recon=None, trivial_mask="this", recon_mask="next", count_columns=True):
    """[trivial, trivial_count, recon, recon_count] in float64.  The defaults are the contract; trivial_mask='next',
    recon_mask='this' and count_columns=False are the wrong variants."""
    x = np.asarray(x, dtype=np.float64)
    B, T, d = x.shape
    len_b = clamp_lengths(lengths, B, T)
    t = np.arange(max(T - 1, 0))[None, :]
    keep = {"this": t < len_b[:, None], "next": t + 1 < len_b[:, None]}                 # [B, T - 1]
    per = d if count_columns else 1
    out = np.zeros(4)
    m = keep[trivial_mask]
    out[1] = per * m.sum()
    out[0] = ((x[:, :-1][m] - x[:, 1:][m]) ** 2).sum() / (out[1] + 1e-8)
    if recon is not None:
        r = np.asarray(recon, dtype=np.float64)
        m = keep[recon_mask]
        out[3] = per * m.sum()
        out[2] = ((r[:, :-1][m] - x[:, 1:][m]) ** 2).sum() / (out[3] + 1e-8)
    return out


def reference_fp32(x, lengths, recon=None):
    """(trivial_loss, recon_loss or None) as train.py:404-424 forms them: fp32, the mask multiplied in, numpy's pairwise sums.
    T >= 2."""
    x = np.asarray(x, dtype=np.float32)
    B, T, d = x.shape
    mask = (np.arange(T)[None, :] < np.asarray(lengths).reshape(-1, 1)).astype(np.float32)
    mexp = np.broadcast_to(mask[:, :, None], x.shape)
    one = np.float32(1e-8)
    tri = ((x[:, :-1] - x[:, 1:]) ** 2 * mexp[:, :-1]).sum(dtype=np.float32) / (mexp[:, :-1].sum(dtype=np.float32) + one)
    rec = None
    if recon is not None:
        r = np.asarray(recon, dtype=np.float32)
        rec = ((r[:, :-1] - x[:, 1:]) ** 2 * mexp[:, 1:]).sum(dtype=np.float32) / (mexp[:, 1:].sum(dtype=np.float32) + one)
    return tri, rec
