"""The cases of the MirrorDescentEstimator tests and a plain numpy restatement of the algorithm (include/pgmhip.h
"Junction-tree potentials by mirror descent") in float64 or longdouble.  The calibration is brute force: the joint
log-table is the broadcast sum of the clique tables, its softmax times n is summed down to every clique.

A case is a dict: card[v]; cliques and marginals, tuples of variable indices; edges, pairs of clique indices; theta,
one log-potential table per clique; targets [B][n_y] and totals [B]; metric, iterations, stepsize (as `estimate`
reads it).  Inside `run` every table is kept "wide": shaped over all the variables, size 1 where it has none.
"""
import functools

import numpy as np

LD = np.longdouble


def run(case, row=0, dtype=np.float64, iterations=None, theta=None):
    """{theta, mu (flat, clique after clique), loss, alpha, trials, rejected, exhausted (iterations whose 25 trials
    were all rejected), armijo [(lhs, rhs)], d_min (the smallest |d_j| met)}"""
    f, card, cliques, marginals = dtype, case["card"], case["cliques"], case["marginals"]
    nv, metric, stepsize = len(card), case["metric"], case["stepsize"]

    def wide(t, scope):
        shape = [card[v] if v in scope else 1 for v in range(nv)]
        return np.transpose(np.asarray(t, dtype=f), np.argsort(scope)).reshape(shape)

    def narrow(t, scope):  # summed down to `scope`, in its order
        t = t.sum(axis=tuple(v for v in range(nv) if v not in scope))
        return np.transpose(t, np.argsort(np.argsort(scope)))

    sizes = [int(np.prod([card[v] for v in m])) for m in marginals]
    y = [wide(t.reshape([card[v] for v in m]), m) for t, m in zip(np.split(np.asarray(case["targets"][row], dtype=f), np.cumsum(sizes)[:-1]), marginals)]
    owner = [next(i for i, c in enumerate(cliques) if set(m) <= set(c)) for m in marginals]
    n = f(case["totals"][row])
    start = case["theta"] if theta is None else np.split(theta, np.cumsum([int(np.prod([card[v] for v in c])) for c in cliques])[:-1])
    th = [wide(np.reshape(t, [card[v] for v in c]), c) for t, c in zip(start, cliques)]
    d_min = [np.inf]

    def calibrate(th):
        joint = functools.reduce(np.add, th)
        top = joint.max()
        logz = top + np.log(np.exp(joint - top).sum())
        full = np.exp(joint + np.log(n) - logz)
        return [wide(narrow(full, c), c) for c in cliques]

    def loss_of(mu):
        loss, dL = f(0), [np.zeros([card[v] if v in c else 1 for v in range(nv)], dtype=f) for c in cliques]
        for j, m in enumerate(marginals):
            d = wide(narrow(mu[owner[j]], m), m) - y[j]
            d_min[0] = min(d_min[0], float(np.abs(d).min()))
            if metric == "L2":
                loss, g = loss + f(0.5) * (d * d).sum(), d
            elif metric == "L1":
                loss, g = loss + np.abs(d).sum(), np.sign(d)
            else:
                raise ValueError("Metric must be one of L1 or L2.")
            dL[owner[j]] = dL[owner[j]] + g
        return loss, dL

    line_search = stepsize is None
    alpha = f(stepsize if isinstance(stepsize, float) else 1.0 / (float(n) * float(n)))
    mu = calibrate(th)
    answer = loss_of(mu)
    trials, rejected, exhausted, armijo = 0, 0, 0, []
    for _ in range(case["iterations"] if iterations is None else iterations):
        omega, nu, (curr, dL) = th, mu, answer
        if line_search:
            alpha = alpha * 2
        for _ in range(25):
            th = [o - alpha * g for o, g in zip(omega, dL)]
            mu = calibrate(th)
            answer = loss_of(mu)
            trials += 1
            lhs, rhs = curr - answer[0], f(0.5) * alpha * sum((g * (a - b)).sum() for g, a, b in zip(dL, nu, mu))
            if line_search:
                armijo.append((float(lhs), float(rhs)))
            if not line_search or lhs >= rhs:
                break
            alpha, rejected = alpha * f(0.5), rejected + 1
        else:
            exhausted += 1
    flat = lambda ts: np.concatenate([narrow(t, c).ravel() for t, c in zip(ts, cliques)])
    return dict(theta=flat(th), mu=flat(mu), loss=answer[0], alpha=float(alpha), trials=trials, rejected=rejected,
                exhausted=exhausted, armijo=armijo, d_min=d_min[0])


@functools.lru_cache(maxsize=None)
def reference(name, row=0):
    """(the longdouble run, the case's figures: the largest float64-against-longdouble difference of mu / n and of
    theta / max(1, |theta|)).  Computed once per case and row."""
    lo, hi = run(CASES[name], row), run(CASES[name], row, dtype=LD)
    scale = max(1.0, float(np.abs(hi["theta"]).max()))
    fig = max(float(np.abs(lo["mu"] - hi["mu"]).max()) / float(CASES[name]["totals"][row]), float(np.abs(lo["theta"] - hi["theta"]).max()) / scale)
    return hi, fig, scale


def tolerance(name, row=0):
    """8 x the case's figure, as tests/test_lbp_gpu.py takes it, and no less than 8 x 2^-52 per calibration of the
    chain (an unlucky float64 run can round to the longdouble one): relative to n for mu, to max(1, |theta|) for theta."""
    hi, fig, scale = reference(name, row)
    return 8 * max(fig, 2.0 ** -52 * (1 + hi["trials"])), scale


def make(card, cliques, edges, marginals, seed, n=20.0, rows=1, metric="L2", iterations=12, stepsize=None, spread=1.0):
    """Random start potentials in [-spread, spread] and targets: the marginals of a random joint, scaled to n (n, 1.3 n,
    .. for more rows) and perturbed so that no clique-consistent table matches them exactly."""
    rng = np.random.default_rng(seed)
    theta = [rng.uniform(-spread, spread, [card[v] for v in c]) for c in cliques]
    targets, totals = [], []
    for b in range(rows):
        joint = rng.dirichlet(np.ones(int(np.prod(card)))).reshape(card)
        total = n * (1 + 0.3 * b)
        row = []
        for m in marginals:
            t = joint.sum(axis=tuple(v for v in range(len(card)) if v not in m))
            t = np.transpose(t, np.argsort(np.argsort(m))).ravel() * rng.uniform(0.9, 1.1, t.size)
            row.append(t / t.sum() * total)
        targets.append(np.concatenate(row)), totals.append(total)
    return dict(card=list(card), cliques=cliques, edges=edges, marginals=marginals, theta=theta, targets=np.array(targets),
                totals=np.array(totals), metric=metric, iterations=iterations, stepsize=stepsize)


def counts(card, marginals, rows):
    """The marginals' contingency tables of data rows (tuples of states), flat."""
    data = np.array(rows)
    return np.concatenate([np.bincount(np.ravel_multi_index([data[:, v] for v in m], [card[v] for v in m]),
                                       minlength=int(np.prod([card[v] for v in m]))) for m in marginals]).astype(float)[None, :]


def fixed(card, cliques, edges, marginals, targets, total, theta, **kw):
    return dict(dict(card=card, cliques=cliques, edges=edges, marginals=marginals, theta=theta, targets=np.asarray(targets, dtype=float),
                     totals=np.array([float(total)]), metric="L2", iterations=8, stepsize=None), **kw)


STAR = ([2, 2, 2, 2, 2], [(0, 1), (1, 2), (2, 3), (2, 4)], [(0, 1), (1, 2), (1, 3)])  # the reference's ab - bc, bc - cd, bc - ce
STAR_ROWS = [(1, 0, 1, 1, 0), (0, 1, 1, 0, 0), (0, 0, 0, 0, 0), (1, 1, 0, 1, 1), (1, 1, 1, 1, 1)]
STAR_ONES = [np.ones((2, 2)) for _ in range(4)]
TWO = ([2, 3, 4, 2], [(0, 1, 2), (2, 1, 3)], [(0, 1)])  # the separator (b, c) in another order on each side
AB = ([2, 3], [(0, 1)], [])
HOT = [np.array([[700.0, 699.0, -700.0], [-700.0, 699.5, 698.0]]), np.array([[700.0, -700.0], [698.5, 699.0], [-699.0, 700.0]])]


def star(marginals, **kw):
    return fixed(*STAR, marginals, counts(STAR[0], marginals, STAR_ROWS), 5, STAR_ONES, **kw)


one = lambda **kw: fixed([2], [(0,)], [], [(0,)], [[30.0, 70.0]], 100, [np.zeros(2)], **kw)
CASES = {
    # 1. one clique of one binary variable; an int step is no line search and alpha = 1 / n^2 (the reference's test)
    "one_l1_int": one(metric="L1", iterations=2, stepsize=1),
    "one_l2_int": one(iterations=2, stepsize=1),
    "one_fixed": one(iterations=5, stepsize=0.1),
    "one_zero": one(iterations=2, stepsize=0.0),  # a float is used as it stands: alpha = 0, and a negative one
    "one_negative": one(iterations=2, stepsize=-0.05),
    "one_search": one(),
    # 2. one clique (a, b) of 2 x 3: a leading stride, a non-leading stride, the whole clique
    "ab_a": make(*AB, [(0,)], seed=1),
    "ab_b": make(*AB, [(1,)], seed=2),
    "ab_ab": make(*AB, [(0, 1)], seed=3),
    # 3. the star: every clique a marginal; unary marginals of the non-root cliques; bc owns two and ab, cd own none
    "star_cliques": star(STAR[1]),
    "star_unary": star([(2,), (3,), (4,)]),
    "star_two_none": star([(2,), (1, 2), (4,)]),
    # 4. two cliques of three variables
    "two": make(*TWO, [(0, 2), (3, 1), (1,)], seed=4),
    # 5. a separator of 65 cells with a residual of 65 (a wave per cell; over 64 KiB of LDS); a table of 16 x 17 cells
    "wave65": make([65, 65, 2], [(0, 1), (1, 2)], [(0, 1)], [(1,), (2, 1)], seed=5, iterations=4),
    "block272": make([16, 17, 3], [(0, 1), (1, 2)], [(0, 1)], [(0,), (1, 2)], seed=6, iterations=6),
    # 6. start potentials near +-700: exp of a sum of two of them overflows, log space stays finite
    "hot": dict(make([2, 3, 2], [(0, 1), (1, 2)], [(0, 1)], [(0, 1), (2,)], seed=7), theta=HOT),
    # 7. rejected trials (L1 gives them readily; most of the line-search cases above hold some too).  No case reaches 25
    #    rejections in one iteration: none was found
    "l1_rejects": make(*TWO, [(0, 2), (3, 1), (1,)], seed=8, metric="L1"),
    "l1_one_clique": make(*AB, [(0,)], seed=9, metric="L1"),
    # 8. three rows of targets with their own totals
    "batch": make(*TWO, [(0, 2), (3, 1), (1,)], seed=10, rows=3),
    # a fixed float step on two cliques (10., the warm start, runs on the star through the estimator: test_md_gpu.py)
    "warm": make(*TWO, [(0, 2), (3, 1), (1,)], seed=11, iterations=5, stepsize=0.01),
}
SEARCH = sorted(k for k, c in CASES.items() if c["stepsize"] is None)
GLOBAL_TIER = ["star_cliques", "star_unary", "star_two_none", "two", "wave65", "block272"]  # 9. again with the global tier forced
