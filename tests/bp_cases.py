"""Case table of the batched calibration schedule (pgmpy_amd/inference/bp_batch.py: BPSchedule).  A plain
module (numpy only) shared by tests/test_bp_cases_cpu.py (the trees, the reference and the bound, no device)
and tests/test_bp_paths_gpu.py (every tree calibrated on the GPU, the branches of the schedule asserted).

Trees.  Small synthetic junction trees (cardinalities 1..4, at most 25 cliques of at most 256 states), each
built for the branches of BPSchedule named in its `want`: entries of BPSchedule.trace the tree must reach at
every row count (`want["any"]`), where the fused product + marginal kernel takes the passes (`want["fused"]`)
and where it declines them (`want["unfused"]`).  The kernel (pgmi_plan_product_marg) takes a pass only when
the row count is even and at least 64, whatever the clique, and product_n_bind / the marginal-only bind go
through the same plan: FUSED_ROWS(n) says which regime a row count is in.  The first clique is the root.

Potentials.  Uniform in [0.05, 1.05) with about 20 % hard zeros; three planted assignments of all variables
(the witnesses) keep every entry they touch positive, and one slice psi_c[u = s_u, v = s_v] that no witness
touches is zeroed, so the evidence {u: s_u, v: s_v} (the tree's `impossible`) has total mass 0 and every
pattern taken from a witness has mass > 0.  With at most 25 cliques the smallest positive product is above
0.05^25 > 1e-33: no underflow.

Evidence.  A tree has fixed evidence columns `ev_vars` (none for chain3_noev, separator variables only for
chain3_sepev); `patterns(tree)` lists the distinct findings (no finding; the impossible pair; every column;
the columns private to leaf cliques; each column alone; random subsets, states from a witness) and row r of a
batch carries pattern r mod len(patterns).

Reference.  Independent of any message schedule: the calibrated belief of clique C is the marginal (sum) or
max-marginal (max) onto C of the product of every clique potential and every finding's indicator, computed
in np.longdouble by eliminating the other variables one at a time (einsum product of the factors holding the
variable, then sum / max over it; max distributes over products of non-negative numbers), all patterns at
once along a pattern axis the indicators carry.  A sepset belief is that belief reduced onto the separator, a
variable's marginal the belief of the first clique holding it summed onto the variable and divided by its
total (NaN where the total is 0).

Bound.  Every input is non-negative, so nothing cancels and the relative error of a result is at most the
number of roundings on the longest path into it, times u = 2^-53, to first order: a product of m operands
costs m - 1 roundings in any association (_aggregate and Program.product_n's balanced tree only regroup it),
a sum of n non-negative terms n - 1 in any order, with or without FMA, a ratio 2 (the division and the
multiplication by it), a max none.  Clique j's pass multiplies m_j = 1 + findings_j + children_j + 2 operands
(its potential, its findings, its child messages, sigma' and mu) and reduces at most r_j = max over its
separators S of |C_j| / |S| terms (0 for max); every clique's pass can enter any belief once in collect and
once in distribute, so

    |got - ref| <= (2 sum_j (m_j + r_j) + 2) u |ref|                    (beliefs and sepset beliefs)

the + 2 for the reference's own rounding to fp64 and the second-order terms (k^2 u^2 with k < 10^4).  A
sepset belief rebuilt from a stored ratio (_SepFromRatio: (sigma' / mu) x mu) is two roundings past sigma',
which the pass's "+ 2" operands already count.  A variable's marginal m / z sums |C| / card beliefs (each
within B = the bound above) onto the variable, then card of those into z, then divides: numerator and
denominator are each within B plus their sums' roundings, so

    |got - ref| <= (2 B / u + 2 |C| / card + card) u |ref|               (marginals)

Entries whose reference is 0 are products with a zero factor in every term: exactly 0 on the device too.
"""
import numpy as np

LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 2.0 ** -60  # 80-bit extended or better
U = 2.0 ** -53
N_WITNESS = 3
N_RANDOM = 6
ZERO_FRACTION = 0.2

# the names of BPSchedule.trace (the decision table of the schedule)
TRACE_NAMES = (
    "ops_direct", "ops_aggregated", "ops_ones", "msg_from_inputs",
    "single_clique", "root_premarginal", "leaf", "inner",
    "ratio_stored", "ratio_blocked_nested_scope", "ratio_not_single_child", "ratio_declined_by_kernel",
    "ratio_knob_off",
    "sigma_from_premarginal", "sigma_via_ratio", "sigma_from_operands", "sigma_pair_from_operands",
    "sigma_pair_from_container", "sigma_contract_from_container", "sigma_contract_from_belief",
    "fin_ratio_operand", "fin_ratio_folded", "fin_sigma_mu_pair", "fin_sigma_mu_folded",
)
# one more decision the schedule takes, outside that table: the single child's message is inside an aggregate
EXTRA_NAMES = ("ratio_message_aggregated",)
# where a name can occur: only when the fused kernel takes the pass; only when it declines one (every pass at
# an odd or short row count, a pass of more than 8 operands at any); only with the knob
FUSED_ONLY = {"ratio_stored", "sigma_via_ratio", "sigma_from_operands", "sigma_pair_from_operands",
              "sigma_pair_from_container", "fin_ratio_operand", "fin_ratio_folded"}
UNFUSED_ONLY = {"ratio_declined_by_kernel", "sigma_contract_from_belief"}
KNOB_ONLY = {"ratio_knob_off"}


def FUSED_ROWS(n_rows):
    """Whether the fused product + marginal kernel takes passes at this row count (pgmi_plan_product_marg:
    the row axis is read two rows per lane, from 64 rows up)."""
    return n_rows >= 64 and n_rows % 2 == 0


def prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


# ----------------------------------------------------------------------------- trees
def _tree(name, cliques, edges, card, ev_vars, impossible, seed, always=(), fused=(), unfused=()):
    """cliques: tuples of variable names, the first one the root; edges: pairs of clique indices;
    impossible: (clique index, u, v) — the pair of evidence columns whose slice is zeroed, or None."""
    cliques = [tuple(c) for c in cliques]
    edges = [(cliques[i], cliques[j]) for i, j in edges]
    card = dict(card)
    variables = sorted(card)
    assert set(variables) == {v for c in cliques for v in c}, name
    rng = np.random.default_rng(seed)
    witness = [{v: int(rng.integers(card[v])) for v in variables} for _ in range(N_WITNESS)]
    pots = {}
    for c in cliques:
        shape = [card[v] for v in c]
        val = rng.random(shape) + 0.05
        zero = rng.random(shape) < ZERO_FRACTION
        for w in witness:
            zero[tuple(w[v] for v in c)] = False
        val[zero] = 0.0
        pots[c] = val
    imp = {}
    if impossible is not None:
        ci, u, v = impossible
        c = cliques[ci]
        assert u in c and v in c and u in ev_vars and v in ev_vars, name
        taken = {(w[u], w[v]) for w in witness}
        su, sv = next((a, b) for a in range(card[u]) for b in range(card[v]) if (a, b) not in taken)
        sl = [slice(None)] * len(c)
        sl[c.index(u)], sl[c.index(v)] = su, sv
        pots[c][tuple(sl)] = 0.0
        imp = {u: su, v: sv}
    return dict(name=name, cliques=cliques, edges=edges, card=card, variables=variables, pots=pots,
                ev_vars=list(ev_vars), impossible=imp, witness=witness, seed=seed,
                want={"any": set(always), "fused": set(fused), "unfused": set(unfused)})


def _chain3(name, ev_vars, impossible, seed, **want):
    return _tree(name, [("a", "b"), ("b", "c"), ("c", "d")], [(0, 1), (1, 2)],
                 dict(a=2, b=3, c=4, d=2), ev_vars, impossible, seed, **want)


def _nested(name, seps, seed, **want):
    """Root (a, b, c, d) with one child per separator in `seps` (the child adds a variable of its own)."""
    card = dict(a=2, b=3, c=2, d=4)
    cliques = [("a", "b", "c", "d")]
    for i, s in enumerate(seps):
        own = "efghi"[i]
        card[own] = 2 + i % 3
        cliques.append(tuple(s) + (own,))
    return _tree(name, cliques, [(0, i) for i in range(1, len(cliques))], card, ["a", "b", "e", "g"], (0, "a", "b"),
                 seed, **want)


def _star7(name, twin, seed, **want):
    """Root (p, x); a hub over x and seven more binary variables, each shared with one child of the hub;
    `twin`: a second child of the root over the same separator {x}."""
    hs = [f"h{i}" for i in range(1, 8)]
    card = dict(p=3, x=2, **{h: 2 for h in hs})
    cliques = [("p", "x"), ("x",) + tuple(hs)]
    edges = [(0, 1)]
    for i, h in enumerate(hs):
        z = f"z{i + 1}"
        card[z] = 2 + i % 3
        cliques.append((h, z))
        edges.append((1, len(cliques) - 1))
    if twin:
        card["q"] = 4
        cliques.append(("x", "q"))
        edges.append((0, len(cliques) - 1))
    return _tree(name, cliques, edges, card, ["p", "x", "z1", "z2", "z5"], (0, "p", "x"), seed, **want)


def _star6():
    """Root (p, x); a hub (x, f1, h1, h2, h3) with findings on f1 and h2 and four children, two of them over
    {h1}, one over {h2} (its message shares the scope of the finding on h2), one over {h3}."""
    card = dict(p=2, x=2, f1=3, h1=2, h2=3, h3=2, z1=2, z2=3, z3=2, z4=4)
    cliques = [("p", "x"), ("x", "f1", "h1", "h2", "h3"), ("h1", "z1"), ("h1", "z2"), ("h2", "z3"), ("h3", "z4")]
    return _tree("star6", cliques, [(0, 1), (1, 2), (1, 3), (1, 4), (1, 5)], card, ["f1", "h2", "p", "z4"],
                 (1, "f1", "h2"), 61,
                 always={"ops_aggregated", "msg_from_inputs", "inner", "ratio_message_aggregated", "fin_sigma_mu_pair"},
                 fused={"ratio_stored", "sigma_via_ratio", "fin_ratio_operand"},
                 unfused={"ratio_declined_by_kernel", "sigma_contract_from_belief"})


def _fan20():
    """Root (r, x, y) with 20 children over {x} and 3 over {x, y}: the 20 messages (and the finding on x) are
    one balanced-tree product over {x}, folded into the {x, y} group."""
    card = dict(r=2, x=3, y=2)
    cliques = [("r", "x", "y")]
    for i in range(20):
        card[f"z{i}"] = 2 + i % 3
        cliques.append(("x", f"z{i}"))
    for i in range(3):
        card[f"w{i}"] = 2 + i % 2
        cliques.append(("x", "y", f"w{i}"))
    return _tree("fan20", cliques, [(0, i) for i in range(1, len(cliques))], card,
                 ["x", "y", "z0", "z7", "z19", "w1"], (0, "x", "y"), 71,
                 always={"ops_aggregated", "root_premarginal", "ratio_not_single_child", "sigma_from_premarginal",
                      "sigma_contract_from_container", "fin_sigma_mu_pair", "ops_direct", "leaf"})


def _deep():
    """Depth 6 with side branches, cardinalities 1..4 (u has one state), a child that lists its separator in
    the other order ((f, d, l) under (d, e, f)), findings on separator variables (each goes to the first
    clique holding the variable)."""
    card = dict(a=2, b=3, c=2, d=4, e=2, f=3, g=2, h=4, i=3, j=2, k=3, l=2, m=4, u=1)
    cliques = [("a", "b", "c"), ("b", "c", "d"), ("c", "d", "e", "u"), ("d", "e", "f"), ("e", "f", "g"),
               ("f", "g", "h"), ("g", "h", "i"), ("a", "j"), ("d", "u", "k"), ("f", "d", "l"), ("e", "m")]
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (0, 7), (2, 8), (3, 9), (4, 10)]
    return _tree("deep", cliques, edges, card, ["c", "d", "e", "f", "g", "u", "i"], (3, "d", "e"), 81,
                 always={"ops_direct", "ops_ones", "root_premarginal", "inner", "leaf", "fin_sigma_mu_pair"},
                 fused={"ratio_stored", "sigma_via_ratio", "fin_ratio_operand"},
                 unfused={"ratio_declined_by_kernel", "sigma_contract_from_belief"})


def _pairs():
    """Root (a, b, c, d, e) whose children's separators come out two per pass once the pass has 256 blocks
    (PAIR_ROWS rows): {a, b, e} and {a, c, e} from the root's operands (8 common states x 32 row blocks),
    {a, b, c} and {a, b, d} from the container {a, b, c, d} (16 x 32)."""
    card = dict(a=4, b=4, c=2, d=2, e=2)
    cliques = [("a", "b", "c", "d", "e")]
    for i, s in enumerate(["abcd", "abe", "abc", "abd", "ace"]):
        card["vwxyz"[i]] = 2
        cliques.append(tuple(s) + ("vwxyz"[i],))
    return _tree("pairs", cliques, [(0, i) for i in range(1, 6)], card, ["a", "e", "v", "z"], (0, "a", "e"), 95,
                 always={"ratio_blocked_nested_scope", "sigma_from_premarginal", "fin_sigma_mu_pair"},
                 fused={"sigma_from_operands"}, unfused={"sigma_contract_from_belief", "sigma_contract_from_container"})


PAIR_ROWS = 16384  # the fewest rows (a power of two) at which both two-marginal passes of `pairs` have 256 blocks
PAIR_NAMES = {"sigma_pair_from_operands", "sigma_pair_from_container"}


def _build():
    ratio = dict(fused={"ratio_stored", "sigma_via_ratio", "fin_ratio_operand"},
                 unfused={"ratio_declined_by_kernel", "sigma_from_premarginal", "fin_sigma_mu_pair"})
    trees = [
        _tree("single", [("a", "b", "c")], [], dict(a=2, b=3, c=4), ["a", "b", "c"], (0, "a", "b"), 11,
              always={"single_clique", "ops_direct"}),
        _chain3("chain3", ["a", "b", "c"], (0, "a", "b"), 21,
                always={"ops_direct", "ops_ones", "root_premarginal", "inner", "leaf"}, **ratio),
        _chain3("chain3_noev", [], None, 22, always={"ops_ones", "root_premarginal", "inner", "leaf"}, **ratio),
        _chain3("chain3_sepev", ["b", "c"], (1, "b", "c"), 23, always={"ops_direct", "ops_ones"}, **ratio),
        # two children over {b, c} and a third that lists the same separator as (c, b): its sigma' is a
        # transposing copy of the premarginal
        _tree("twins", [("a", "b", "c"), ("b", "c", "d"), ("b", "c", "e"), ("c", "b", "f")],
              [(0, 1), (0, 2), (0, 3)], dict(a=2, b=3, c=4, d=2, e=3, f=2), ["a", "d", "e", "b"], (0, "a", "b"), 31,
              always={"root_premarginal", "ratio_not_single_child", "sigma_from_premarginal", "fin_sigma_mu_pair",
                   "sigma_contract_from_container", "leaf"}),
        _nested("nested", ["abc", "ab", "bc", "cd", "ad"], 41,
                always={"ops_direct", "ratio_blocked_nested_scope", "sigma_from_premarginal", "fin_sigma_mu_pair"},
                # (the two-marginal pass needs 256 blocks: at these row counts each marginal is a pass of its own)
                fused={"sigma_from_operands", "sigma_contract_from_container"},
                unfused={"sigma_contract_from_container", "sigma_contract_from_belief"}),
        _nested("nested_single", ["abc", "ab", "cd"], 42,
                always={"ratio_blocked_nested_scope", "sigma_from_premarginal", "sigma_contract_from_container"},
                fused={"sigma_from_operands"}, unfused={"sigma_contract_from_belief"}),
        # the hub's finalising pass has 9 operands (its potential, 7 messages, the ratio): more than the fused
        # kernel takes at any row count, so its own premarginal and its children's sigma' are declined
        _star7("star7_ratio", False, 51,
               always={"ops_aggregated", "inner", "ratio_declined_by_kernel", "sigma_contract_from_belief"},
               fused={"ratio_stored", "sigma_via_ratio", "fin_ratio_folded"},
               unfused={"fin_sigma_mu_folded"}),
        _star7("star7_sigma", True, 52,
               always={"ops_aggregated", "ratio_not_single_child", "sigma_from_premarginal", "fin_sigma_mu_folded",
                    "fin_sigma_mu_pair", "ratio_declined_by_kernel", "sigma_contract_from_belief"}),
        _star6(),
        _fan20(),
        _deep(),
        # the child lists the separator {b, c} (equal cardinalities) in the other order than its parent: a
        # ratio stored in the parent's order and read in the child's would pass every shape check
        _tree("chain_swapped", [("a", "b", "c"), ("c", "b", "d")], [(0, 1)], dict(a=2, b=3, c=3, d=2),
              ["a", "b", "d"], (0, "a", "b"), 91, always={"root_premarginal", "leaf"},
              fused={"ratio_stored", "sigma_via_ratio", "fin_ratio_operand"},
              unfused={"ratio_declined_by_kernel", "sigma_contract_from_container", "fin_sigma_mu_pair"}),
        _pairs(),
    ]
    return {t["name"]: t for t in trees}


TREES = _build()


# ----------------------------------------------------------------------------- structure
def rooted(tree):
    """(order, parent, children): breadth-first edges (parent, child) from the first clique, as
    BatchedJunctionTree orders them."""
    adj = {c: [] for c in tree["cliques"]}
    for a, b in tree["edges"]:
        adj[a].append(b)
        adj[b].append(a)
    root = tree["cliques"][0]
    order, seen, queue = [], {root}, [root]
    while queue:
        p = queue.pop(0)
        for c in adj[p]:
            if c not in seen:
                seen.add(c)
                order.append((p, c))
                queue.append(c)
    parent = {c: p for p, c in order}
    children = {c: [k for p, k in order if p == c] for c in tree["cliques"]}
    return order, parent, children


def first_clique(tree, var):
    return next(c for c in tree["cliques"] if var in c)


def running_intersection(tree):
    """Every variable's cliques form a connected subtree, and the edges form a tree over all cliques."""
    order, parent, _ = rooted(tree)
    if len(order) != len(tree["cliques"]) - 1 or len(tree["edges"]) != len(order):
        return False
    for v in tree["variables"]:
        holds = [c for c in tree["cliques"] if v in c]
        tops = [c for c in holds if c not in parent or v not in parent[c]]
        if len(tops) != 1:
            return False
    return True


# ----------------------------------------------------------------------------- evidence
def patterns(tree):
    """The distinct findings of a tree's batches, {variable: state} each; [0] none, [1] the impossible pair
    (when the tree has evidence columns)."""
    ev = tree["ev_vars"]
    if not ev:
        return [{}]
    w = tree["witness"]
    _, parent, children = rooted(tree)
    inner = {v for c in tree["cliques"] if children[c] for v in c}
    out = [{}, dict(tree["impossible"]), {v: w[0][v] for v in ev}, {v: w[1][v] for v in ev if v not in inner}]
    out += [{v: w[2][v]} for v in ev]
    rng = np.random.default_rng(tree["seed"] + 1000)
    for _ in range(N_RANDOM):
        k = int(rng.integers(N_WITNESS))
        out.append({v: w[k][v] for v in ev if rng.random() < 0.5})
    return out


def codes(tree, n_rows, shift=0):
    """uint8 [max(1, columns), n_rows] evidence codes (255 = no finding): row r carries pattern
    (r + shift) mod len(patterns)."""
    pats = patterns(tree)
    ev = tree["ev_vars"]
    out = np.full((max(1, len(ev)), n_rows), 255, dtype=np.uint8)
    for r in range(n_rows):
        for v, s in pats[(r + shift) % len(pats)].items():
            out[ev.index(v), r] = s
    return out


def row_patterns(tree, n_rows, shift=0):
    return (np.arange(n_rows) + shift) % len(patterns(tree))


# ----------------------------------------------------------------------------- reference
PAT = "\0pattern"  # the pattern axis of the indicators


def _eliminate(factors, keep, card, op):
    """Sum / max out every variable not in `keep` from the product of `factors` [(labels, LD array)];
    returns the array over keep (+ the pattern axis last, when a factor carries it)."""
    factors = list(factors)
    todo = {v for ls, _ in factors for v in ls} - set(keep) - {PAT}

    def combine(bucket, drop):
        labels = []
        for ls, _ in bucket:
            labels += [v for v in ls if v not in labels]
        ix = {v: i for i, v in enumerate(labels)}
        (l0, full), rest = bucket[0], bucket[1:]
        l0 = list(l0)
        for ls, a in rest:  # two operands at a time: einsum's operand count is limited
            l1 = l0 + [v for v in ls if v not in l0]
            full = np.einsum(full, [ix[v] for v in l0], a, [ix[v] for v in ls], [ix[v] for v in l1])
            l0 = l1
        assert full.dtype == LD and l0 == labels
        if drop is None:
            return labels, full
        ax = labels.index(drop)
        return [v for v in labels if v != drop], (full.sum(axis=ax) if op == "sum" else full.max(axis=ax))

    while todo:
        def cost(v):
            seen = set()
            for ls, _ in factors:
                if v in ls:
                    seen.update(ls)
            return prod(card.get(x, 1) for x in seen if x != PAT)

        v = min(sorted(todo), key=cost)
        bucket = [f for f in factors if v in f[0]]
        factors = [f for f in factors if v not in f[0]] + [combine(bucket, v)]
        todo.discard(v)
    labels, full = combine(factors, None)
    want = list(keep) + ([PAT] if PAT in labels else [])
    return np.transpose(full, [labels.index(v) for v in want])


_REF = {}


def reference(tree, op):
    """Closed-form calibration of every pattern of the tree, computed once per (tree, op) and shared.
    op: "sum" or "max".  Returns dict(beliefs={clique: LD [patterns, prod card]}, seps={(parent, child):
    (LD [patterns, prod sep card], sep labels in the child's order)}, marginals={var: LD [patterns, card]},
    mass=LD [patterns])."""
    key = (tree["name"], op)
    if key in _REF:
        return _REF[key]
    pats = patterns(tree)
    card = tree["card"]
    factors = [(list(c), tree["pots"][c].astype(LD)) for c in tree["cliques"]]
    for v in tree["ev_vars"]:
        ind = np.ones((card[v], len(pats)), dtype=LD)
        for i, p in enumerate(pats):
            if v in p:
                ind[:, i] = 0
                ind[p[v], i] = 1
        factors.append(([v, PAT], ind))
    order, _, _ = rooted(tree)
    beliefs, full = {}, {}
    for c in tree["cliques"]:
        b = _eliminate(factors, c, card, op)
        if b.ndim == len(c):  # no evidence column: one pattern
            b = b[..., None]
        full[c] = b
        beliefs[c] = np.ascontiguousarray(np.moveaxis(b, -1, 0)).reshape(len(pats), -1)
    seps = {}
    for p, c in order:
        sl = [v for v in c if v in p]
        ax = tuple(i for i, v in enumerate(c) if v not in p)
        s = full[c].sum(axis=ax) if op == "sum" else full[c].max(axis=ax)
        seps[(p, c)] = (np.ascontiguousarray(np.moveaxis(s, -1, 0)).reshape(len(pats), -1), sl)
    marg = {}
    for v in tree["variables"]:
        c = first_clique(tree, v)
        m = full[c].sum(axis=tuple(i for i, x in enumerate(c) if x != v))  # [card, patterns]
        with np.errstate(invalid="ignore", divide="ignore"):
            marg[v] = (m / m.sum(axis=0)).T.copy()
    root = tree["cliques"][0]
    mass = beliefs[root].sum(axis=1) if op == "sum" else beliefs[root].max(axis=1)
    _REF[key] = dict(beliefs=beliefs, seps=seps, marginals=marg, mass=mass)
    return _REF[key]


# ----------------------------------------------------------------------------- bound
def roundings(tree, op):
    """2 sum_j (m_j + r_j) + 2: see the module docstring."""
    _, parent, children = rooted(tree)
    card = tree["card"]
    total = 0
    for c in tree["cliques"]:
        findings = sum(1 for v in tree["ev_vars"] if first_clique(tree, v) == c)
        m = 1 + findings + len(children[c]) + 2
        r = 0
        if op == "sum":
            nbr = children[c] + ([parent[c]] if c in parent else [])
            size = prod(card[v] for v in c)
            r = max([size // prod(card[v] for v in c if v in n) for n in nbr], default=0)
        total += m + r
    return 2 * total + 2


def bound(tree, op):
    """Relative error bound of every clique and sepset belief entry."""
    return roundings(tree, op) * U


def marginal_bound(tree, op, var):
    """Relative error bound of a variable's normalised marginal (summed from the first clique holding it)."""
    c = first_clique(tree, var)
    k = tree["card"][var]
    return (2 * roundings(tree, op) + 2 * (prod(tree["card"][v] for v in c) // k) + k) * U


def check(got, ref, rel, what):
    """Every entry of fp64 `got` against the LD `ref`: exact zeros where ref is 0, NaN where ref is NaN, within
    rel x |ref| elsewhere.  Returns the worst |got - ref| / (rel |ref|)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=LD)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs"
    zero = (ref == 0) & ~nan
    assert np.all(got[zero] == 0), f"{what}: {int(np.count_nonzero(got[zero]))} entries not exactly 0"
    live = ~zero & ~nan
    if not live.any():
        return 0.0
    err = np.abs(got[live].astype(LD) - ref[live]) / (LD(rel) * np.abs(ref[live]))
    worst = float(err.max())
    assert worst <= 1.0, f"{what}: worst error {worst:.3g} x the bound {rel:.3g}"
    return worst
