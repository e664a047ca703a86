"""Oracle of the fused word2vec kernels (k_w2v / k_w2v_ns), shared by
test_w2v_oracle.py and test_gpu_w2v_oracle.py. It is written from the
formulas alone and imports nothing from multiverso_amd: the negative sampler
is Python integers masked to 64 bits, the training step is sequential numpy
float64.

A group is (input rows, output rows with labels). Per group:
    h   = mean of the input rows (0 when there are none)
    per output row w, label y:  f = sigmoid(h.w), e = y - f,
        err += e * w   (the row before its update)
        plain:    w += e * lr * h
        adagrad:  G += (e*h)^2;  w += e*h*lr0/sqrt(G)  where G > 1e-10
    per input row v:
        plain:    v += lr * err
        adagrad:  G += err^2;    v += err*lr0/sqrt(G)  where G > 1e-10
"""

import numpy as np

MASK64 = (1 << 64) - 1
LCG_MUL = 25214903917
LCG_ADD = 11
GSQ_MIN = 1e-10  # adagrad steps only where the accumulator exceeds this


def ns_draws(seed, g, neg, pool_n):
    """The `neg` pool positions group g draws: the stream starts at
    seed + g*MUL + 11 and each draw advances it once more."""
    r = (int(seed) + int(g) * LCG_MUL + LCG_ADD) & MASK64
    out = []
    for _ in range(int(neg)):
        r = (r * LCG_MUL + LCG_ADD) & MASK64
        out.append((r >> 8) % int(pool_n))
    return out


def expand_ns(centers, pool, neg, seed):
    """Ragged (out_idx, out_label, out_off) lists of a negative-sampling
    launch: per group the centre with label 1, then its draws with label 0.
    A draw that lands on the group's own centre is dropped, but it has
    consumed its step of the stream."""
    centers = [int(c) for c in centers]
    pool = [int(p) for p in pool]
    out_idx, out_label, out_off = [], [], [0]
    for g, pos in enumerate(centers):
        out_idx.append(pos)
        out_label.append(1.0)
        for p in ns_draws(seed, g, neg, len(pool)):
            if pool[p] == pos:
                continue
            out_idx.append(pool[p])
            out_label.append(0.0)
        out_off.append(len(out_idx))
    return out_idx, out_label, out_off


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def train(in_buf, out_buf, in_gsq, out_gsq, in_idx, in_off, out_idx,
          out_label, out_off, lr, use_adagrad, lr0):
    """One launch, group by group in float64. The four buffers are copied,
    never written. Returns (in_buf, out_buf, in_gsq, out_gsq, margin); the
    gsq results are None without adagrad, and margin is the smallest
    |G - 1e-10| / 1e-10 over every adagrad mask decision (inf without)."""
    a = np.array(in_buf, dtype=np.float64)
    b = np.array(out_buf, dtype=np.float64)
    ga = np.array(in_gsq, dtype=np.float64) if use_adagrad else None
    gb = np.array(out_gsq, dtype=np.float64) if use_adagrad else None
    in_idx = [int(i) for i in in_idx]
    out_idx = [int(i) for i in out_idx]
    in_off = [int(i) for i in in_off]
    out_off = [int(i) for i in out_off]
    out_label = [float(y) for y in out_label]
    assert len(in_off) == len(out_off)
    dim = a.shape[1]
    margin = float("inf")

    def step(w, G, grad):
        # adagrad update of one row, in place
        nonlocal margin
        G += grad * grad
        margin = min(margin, float(np.min(np.abs(G - GSQ_MIN)) / GSQ_MIN))
        m = G > GSQ_MIN
        w[m] += grad[m] * lr0 / np.sqrt(G[m])

    for g in range(len(in_off) - 1):
        ins = in_idx[in_off[g]:in_off[g + 1]]
        h = np.zeros(dim)
        for r in ins:
            h += a[r]
        if ins:
            h /= len(ins)
        err = np.zeros(dim)
        for o in range(out_off[g], out_off[g + 1]):
            w = b[out_idx[o]]
            e = out_label[o] - _sigmoid(float(h @ w))
            err += e * w
            if use_adagrad:
                step(w, gb[out_idx[o]], e * h)
            else:
                w += e * lr * h
        for r in ins:
            if use_adagrad:
                step(a[r], ga[r], err)
            else:
                a[r] += lr * err
    return a, b, ga, gb, margin
