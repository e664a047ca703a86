"""fp64 oracle and comparison rule for MatrixTable.nearest_rows (not a test
file; tests/test_nearest_rows.py and tests/test_gpu_nearest_rows.py use it).

The oracle computes every query-row score in float64 from the fp32 inputs
with the definitions of nearest_rows: ``dot`` is ``sum_e r[e]*q[e]``;
``cosine`` normalises the query (a zero query stays zero) and divides by the
row's norm, a zero-norm row scoring exactly 0.0; a NaN score counts as -inf.
It also returns ``A = sum_e |q_e||r_e|`` (divided by the norms under cosine).

The tolerance is derived, not tuned: an fp32 dot product of n terms, in any
summation order, errs by at most ``n * 2^-24 * A`` to first order; 8 more
units cover the fused multiply-adds, the ``rr`` sum, the square root, the
divide and the query normalisation:

    tol = (num_col + 8) * 2^-24 * A          per (query, row) pair
"""

import torch

NEG_INF = float("-inf")


def oracle(table: torch.Tensor, queries: torch.Tensor, metric: str):
    """(S, A), each float64 [Q, R]."""
    t = table.detach().cpu().double()
    q = queries.detach().cpu().double().reshape(-1, t.shape[1])
    if metric == "cosine":
        qn = q.norm(dim=1, keepdim=True)
        q = torch.where(qn > 0, q / qn, q)
    S = q @ t.t()
    A = q.abs() @ t.abs().t()
    if metric == "cosine":
        rn = t.norm(dim=1)
        zero = (rn == 0).expand_as(S)
        S = torch.where(zero, torch.zeros_like(S), S / rn)
        A = torch.where(zero, torch.zeros_like(A), A / rn)
    S = torch.where(S.isnan(), torch.full_like(S, NEG_INF), S)
    return S, A


def tolerance(A: torch.Tensor, num_col: int) -> torch.Tensor:
    return (num_col + 8) * 2.0 ** -24 * A


def rank_rows(S: torch.Tensor) -> torch.Tensor:
    """Row ids [Q, R] in the ordering rule's order: score descending, equal
    scores by ascending id."""
    # ids ascend already; a stable descending sort keeps them so among ties
    return torch.sort(S, dim=1, descending=True, stable=True).indices


def oracle_topk(table, queries, k: int, metric: str):
    """(scores fp32 [Q,k], ids int64 [Q,k]): what an exact computation
    returns. Only meaningful to compare bit for bit where fp32 is exact."""
    S, _ = oracle(table, queries, metric)
    ids = rank_rows(S)[:, :k]
    return S.gather(1, ids).float(), ids


def margin(table, queries, k: int, metric: str) -> float:
    """min over queries of g / (2*tol): g the oracle gap between the k-th
    and (k+1)-th score, tol the query's largest pair tolerance. Above 1 the
    id set is determined."""
    S, A = oracle(table, queries, metric)
    if S.shape[1] <= k or S.shape[0] == 0:
        return float("inf")
    top = torch.sort(S, dim=1, descending=True).values
    g = top[:, k - 1] - top[:, k]
    tol = tolerance(A, table.shape[1]).max(dim=1).values
    return float((g / (2 * tol)).min())


def check(result, inputs) -> int:
    """``result`` = (scores [Q,k], ids [Q,k]) from nearest_rows; ``inputs`` =
    (table fp32 [R,C], queries fp32 [Q,C], k, metric). Asserts

    1. ids distinct and in range;
    2. each score within ``tol`` of the oracle score of its id (equal where
       the oracle's is not finite);
    3. the pairs in the ordering rule's order by their own fp32 scores;
    4. per query, with g the oracle gap between its k-th and (k+1)-th score
       and tol the query's largest pair tolerance: if ``g > 2*tol`` the id
       set equals the oracle's, otherwise every returned id has an oracle
       score of at least the k-th oracle score minus ``2*tol``.

    Returns how many queries took the weaker branch of 4."""
    scores, ids = result
    table, queries, k, metric = inputs
    scores = scores.detach().cpu()
    ids = ids.detach().cpu()
    R, C = table.shape
    S, A = oracle(table, queries, metric)
    Q = S.shape[0]
    assert scores.shape == (Q, k) and ids.shape == (Q, k), (scores.shape,
                                                            ids.shape)
    assert scores.dtype == torch.float32 and ids.dtype == torch.int64
    if Q == 0:
        return 0
    tol = tolerance(A, C)
    order = rank_rows(S)
    weaker = 0
    for q in range(Q):
        i, s = ids[q], scores[q].double()
        assert int(i.min()) >= 0 and int(i.max()) < R, (q, i)
        assert i.unique().numel() == k, (q, "duplicate ids", i)
        want, t = S[q, i], tol[q, i]
        fin = want.isfinite()
        assert bool((s[~fin] == want[~fin]).all()), (q, s, want)
        err = (s[fin] - want[fin]).abs()
        assert bool((err <= t[fin]).all()), (
            q, "score off by", float((err / t[fin].clamp_min(1e-300)).max()),
            "of tol")
        for a in range(k - 1):
            sa, sb = float(scores[q, a]), float(scores[q, a + 1])
            assert sa > sb or (sa == sb and int(i[a]) < int(i[a + 1])), (
                q, a, "order", sa, sb, int(i[a]), int(i[a + 1]))
        tq = float(tol[q].max())
        kth = float(S[q, order[q, k - 1]])
        g = kth - float(S[q, order[q, k]]) if R > k else float("inf")
        if g > 2 * tq:
            assert set(i.tolist()) == set(order[q, :k].tolist()), (
                q, "id set", sorted(i.tolist()),
                sorted(order[q, :k].tolist()))
        else:
            weaker += 1
            assert bool((want >= kth - 2 * tq).all()), (q, want, kth, tq)
    return weaker
