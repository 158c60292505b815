"""float64 oracles of the KVzap / DMS tests: the surrogate's score with the `scale` its error bound is written in, the threshold select,
and DMSPress step by step (kvpress/presses/kvzap_press.py:33-45, :79-81; kvpress/presses/dms_press.py:69-130)."""
import numpy as np


def gelu(v):
    """erf GELU in float64 (nn.GELU(), approximate='none')"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()


def kvzap_score(x, w1, b1, w2=None, b2=None):
    """(out, scale), float64 [B, Hout, S] each, from x [B,S,K] and one surrogate layer; w2 None: the linear model.
    scale = |b2| + sum_j |W2_j| (|b1_j| + sum_k |x_k| |W1_jk|)   (linear: |b| + sum_k |x_k| |W_k|)"""
    x, w1, b1 = (np.asarray(a, np.float64) for a in (x, w1, b1))
    pre = x @ w1.T + b1                               # [B, S, N or Hout]
    mag = np.abs(x) @ np.abs(w1).T + np.abs(b1)
    if w2 is None:
        return pre.transpose(0, 2, 1), mag.transpose(0, 2, 1)
    w2, b2 = np.asarray(w2, np.float64), np.asarray(b2, np.float64)
    out = gelu(pre) @ w2.T + b2
    scale = mag @ np.abs(w2).T + np.abs(b2)
    return out.transpose(0, 2, 1), scale.transpose(0, 2, 1)


def worst_ratio(got, ref, scale, factor):
    """max |got - ref| / (factor * scale)"""
    return float((np.abs(np.asarray(got, np.float64) - ref) / (factor * scale)).max())


def threshold_select(scores, threshold, shift=0):
    """(b, h, p + shift) int64 of every score < threshold, row-major (torch.where's order); a NaN is not below anything"""
    with np.errstate(invalid="ignore"):
        b, h, p = np.nonzero(np.asarray(scores) < threshold)
    return b.astype(np.int64), h.astype(np.int64), p.astype(np.int64) + int(shift)


def triples_set(triples):
    return set(zip(*(np.asarray(t).tolist() for t in triples)))


class Dms:
    """DMSPress's bookkeeping for ONE layer, fed with the scores of each forward (dms_press.py:92-128)"""

    def __init__(self, threshold, window, decoding=True):
        self.threshold, self.window, self.decoding = threshold, window, decoding
        self.buffer, self.masked, self.cache_len, self.ratio = None, None, 0, 0

    def step(self, scores, prefilling):
        scores = np.asarray(scores, np.float32)
        if prefilling:
            self.masked, self.cache_len = None, 0          # the attention patch forgets the masks at a prefill
        self.cache_len += scores.shape[-1]
        if not prefilling and not self.decoding:
            return
        self.buffer = scores if prefilling else np.concatenate([self.buffer, scores], axis=-1)
        n = self.buffer.shape[-1] - self.window
        if n > 0:
            new = threshold_select(self.buffer[..., :n], self.threshold, self.cache_len - n - self.window)
            self.buffer = self.buffer[..., n:]
            if len(new[0]):
                self.masked = new if self.masked is None else tuple(np.concatenate([a, c]) for a, c in zip(self.masked, new))
        B, H = scores.shape[:2]
        self.ratio = 0 if self.masked is None else len(self.masked[0]) / (B * H * self.cache_len)
