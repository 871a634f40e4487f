"""Every path of the specialised batch generator (pgmi_cs_bind) against a long-double reference.

tests/nary_cases.py names the paths and holds the cases; tests/test_nary_cases_cpu.py proves on the host which
path each case takes.  Here the cases run as level batches of a plain Program (about 40 jobs per generated
kernel), with signed values, whole slices of zeros and planted special values.  A sum is compared with the
long-double sum of the fp64 terms (the products are a left fold rounded to fp64, which the reference reproduces
exactly) under

    |got - ref| <= (n_red + 2) * 2^-53 * sum |term|,

max, pure products and the elementwise pair combines exactly, the NaN / inf pattern exactly, every output.  The
plan the table claims is checked against the generated source (pgm_pm_bound_source), searching only for the
generator's own identifiers.
"""
import ctypes
import time

import numpy as np
import pytest

from tests import nary_cases as K

pytestmark = pytest.mark.gpu

PER_BATCH = 40
VALUES = ("signed", "zeros", "specials")


def _e():
    from pgmpy_amd import engine

    return engine


def _n():
    from pgmpy_amd import _native

    return _native


def _chunks(xs, n=PER_BATCH):
    k = -(-len(xs) // n)  # equal parts of at most n
    size = -(-len(xs) // k)
    return [xs[i:i + size] for i in range(0, len(xs), size)]


NAMED = _chunks(K.CASES)
RANDOM = _chunks(K.all_random()) + _chunks(K.random_pair_cases(K.RANDOM_PAIR_SEED, K.RANDOM_PAIRS))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _source(bound):
    buf = ctypes.create_string_buffer(1 << 22)
    n = _n().lib().pgm_pm_bound_source(bound, buf, len(buf))
    assert 0 < n < len(buf)
    return buf.value.decode()


def _body(src, j):
    """The generated device function of job j."""
    start = src.index(f" void cj{j}(unsigned tid")
    end = src.find("__device__ __forceinline__ void cj", start)
    return src[start:end if end > 0 else src.index("struct pgm_pm_args")]


def _record(prog, c, ops, view):
    if c["kind"] == "nary":
        return prog.contract_n(list(zip(ops, c["ops"])), c["out"], reduce=c["reduce"], out=view)
    B = ops[1] if len(ops) > 1 else None
    return prog.contract(ops[0], c["ops"][0], B, c["ops"][1] if B is not None else None, c["out"],
                         reduce=c["reduce"], combine=c["combine"], out=view)


class Level:
    """The cases as the jobs of one level batch of a plain Program (one generated kernel)."""

    def __init__(self, cases):
        from pgmpy_amd.program import Program

        self.cases = cases
        self.prog = Program()
        self.items = []
        self.prog.begin_batch()
        for c in cases:
            ops, buf, view = K.make_tensors(c, K.make_values(c, "signed"), "cuda")
            out = _record(self.prog, c, ops, view)
            self.items.append((c, ops, buf, out))
        self.prog.end_batch()
        assert self.prog.check_hazards() == []
        assert all("specialised" in n for n in self.prog.notes), self.prog.notes

    def set(self, values):
        self.arrays = [K.make_values(c, values) for c in self.cases]
        for (c, ops, buf, out), arrays in zip(self.items, self.arrays):
            K.set_values(c, ops, arrays)
        self.clear()

    def clear(self):
        for c, ops, buf, out in self.items:
            (out if buf is None else buf).fill_(K.SENTINEL)

    def results(self):
        import torch

        torch.cuda.synchronize()
        return [out.cpu().numpy() for _, _, _, out in self.items]

    def run(self, values):
        self.set(values)
        self.prog.run()
        return self.results()

    def check(self, got, what):
        worst = 0.0
        for (c, ops, buf, out), arrays, g in zip(self.items, self.arrays, got):
            worst = max(worst, K.compare(c, g, arrays))
            if c["out_kind"] == "pad":
                K.check_sentinels(c, buf.cpu().numpy())
        print(f"{what}: {len(self.items)} jobs, worst |got - ref| / bound = {worst:.3f}")
        return worst


_LEVELS = {}


def _level(key, cases):
    if key not in _LEVELS:
        t0 = time.perf_counter()
        _LEVELS[key] = Level(cases)
        _LEVELS[key].run("signed")  # the first run compiles the generated kernel
        print(f"{key}: recorded, compiled and first run in {time.perf_counter() - t0:.2f} s")
    return _LEVELS[key]


# ----------------------------------------------------------------------------- level batches
@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("batch", range(len(NAMED)))
def test_named_cases_match_reference(gpu, batch, values):
    lv = _level(("named", batch), NAMED[batch])
    lv.check(lv.run(values), f"named batch {batch}, {values}")


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("batch", range(len(RANDOM)))
def test_random_cases_match_reference(gpu, batch, values):
    lv = _level(("random", batch), RANDOM[batch])
    lv.check(lv.run(values), f"random batch {batch}, {values}")


def test_specials_reach_the_outputs(gpu):
    """The planted values are not lost on the way: a batch holds NaN, +inf and -inf outputs, and the one-operand
    marginal's outputs 0 and 1 are NaN (a NaN at the first / the last reduction entry) and output 2 is -inf (its
    whole reduction is)."""
    lv = _level(("named", 0), NAMED[0])
    got = dict(zip([c["name"] for c in lv.cases], lv.run("specials")))
    kinds = np.concatenate([g.reshape(-1) for g in got.values()])
    assert np.isnan(kinds).any() and np.isposinf(kinds).any() and np.isneginf(kinds).any()
    both = [b for b in range(len(NAMED)) if any(c["name"] == "ops1_marginal" for c in NAMED[b])]
    lv = _level(("named", both[0]), NAMED[both[0]])
    g = dict(zip([c["name"] for c in lv.cases], lv.run("specials")))["ops1_marginal"]
    assert np.isnan(g[0]) and np.isnan(g[1]) and g[2] == -np.inf


# ----------------------------------------------------------------------------- the plan, read from the source
def _check_nary_source(c, body):
    p = K.plan_nary(c)
    G, P = p["G"], p["P"]
    assert body.count("__shfl_xor(acc") == p["g_log2"], c["name"]
    assert (f"lane_g = (tid & 63u) / {P}u;" in body) == (1 < G < 64), c["name"]
    assert ("lane_g = tid & 63u;" in body) == (G == 64), c["name"]
    assert (f"out < {p['n_out']}u;" in body), c["name"]
    for t in range(len(c["ops"])):
        assert f"X{t}[" in body, c["name"]
    assert f"X{len(c['ops'])}[" not in body, c["name"]
    if p["nr"] == 0:
        assert "for (unsigned r" not in body, c["name"]
    elif G > 1:
        split = p["sd"] < p["nr"]
        stride_loop = f"#pragma unroll {1 if split else 4}\n    for (unsigned r = lane_g; r < {p['n_red'] // p['inner']}u; r += {G}u)"
        assert stride_loop in body, c["name"]
        assert body.count("for (unsigned r") == 1 + (p["nr"] - p["sd"]), c["name"]
    else:
        assert body.count("for (unsigned r") == p["nr"], c["name"]
    assert ("#pragma unroll 2\n" in body) == p["rolled"], c["name"]
    assert ("pgm_maxn(acc" in body) == (c["reduce"] == "max" and p["nr"] > 0), c["name"]


def _check_pair_source(c, body, ops, out):
    B = ops[1].data_ptr() if len(ops) > 1 else 0
    p = K.plan_pair(c, a_ptr=ops[0].data_ptr(), b_ptr=B, c_ptr=out.data_ptr())
    assert ("double lo = " in body) == (p["row_mode"] == 2), c["name"]
    assert ("const pgm_d2 xa = *(const pgm_d2 *)a_;" in body) == p["va"], c["name"]
    assert ("const pgm_d2 xb = *(const pgm_d2 *)b_;" in body) == p["vb"], c["name"]
    if p["row_mode"] == 0:
        assert body.count("__shfl_xor(acc") == p["g_log2"], c["name"]
        assert f"out < {p['n_out']}u;" in body, c["name"]
    assert body.count("for (unsigned r") == p["outer_loops"] + 1, c["name"]
    assert ("#pragma unroll 1\n" in body) == p["rolled"], c["name"]
    return p


def _check_level_source(lv):
    src = _source(lv.prog._pm_bound[0])
    seen = set()
    for j, (c, ops, buf, out) in enumerate(lv.items):
        body = _body(src, j)
        if c["kind"] == "nary":
            _check_nary_source(c, body)
            seen |= K.classes_nary(c)
        else:
            seen |= K.classes_pair(c, _check_pair_source(c, body, ops, out))
    return src, seen


def test_generated_source_has_the_plan_the_table_claims(gpu):
    """Job by job: the shuffle count is log2 G, the lane map is the plan's, the strided loop covers the outer
    dims the plan splits off, the rolled loops are where the unroll boundary puts them; pair jobs use output
    pairs / vector loads exactly when the restated plan says so on the real addresses.  Every path class of the
    table is seen in a generated kernel."""
    seen = set()
    for b in range(len(NAMED)):
        lv = _level(("named", b), NAMED[b])
        assert len(lv.prog._pm_bound) == 1 and lv.prog.notes == [f"specialised batch of {len(lv.items)}"]
        seen |= _check_level_source(lv)[1]
    assert (K.NARY_CLASSES | K.PAIR_CLASSES) <= seen, (K.NARY_CLASSES | K.PAIR_CLASSES) - seen
    for b in range(len(RANDOM)):
        _check_level_source(_level(("random", b), RANDOM[b]))


# ----------------------------------------------------------------------------- batch forms
def _eight_operand_jobs(n):
    out = []
    for i in range(n):
        q = 2 + i % 5
        out.append(K.nary(f"table8_{i}", dict(p=2 + i % 3, q=q, r=1 + i % 4), ["p", "pr", "r", "p", "q", "rp", "p", "pq"],
                          "q", "max" if i % 7 == 3 else "sum", views=["c", "T", "off", "c", "s2", "c", "c", "s2off"]))
    return out


def test_pointer_table_batch(gpu):
    """60 eight-operand jobs: 540 pointers, over the 512 the kernel arguments hold, so the one generated kernel
    reads its pointers from a table in device memory."""
    lv = Level(_eight_operand_jobs(60))
    for values in ("signed", "specials"):
        lv.check(lv.run(values), f"pointer table, {values}")
    assert lv.prog.notes == ["specialised batch of 60"], lv.prog.notes
    src, _ = _check_level_source(lv)
    assert "const double *const *__restrict__ p;" in src


def test_small_batch_fits_kernel_arguments_and_unbalanced_tree(gpu):
    """5 eight-operand jobs (45 pointers as kernel arguments): the dispatch tree splits 2 | 3."""
    lv = Level(_eight_operand_jobs(5))
    lv.check(lv.run("signed"), "5 jobs")
    src, _ = _check_level_source(lv)
    assert "struct pgm_pm_args { const double *p[45]; };" in src
    assert src.count("if (b < ") == 4


def test_mixed_pair_gather_nary_level(gpu):
    """One level of n-ary, pair and evidence-gather jobs (7 jobs: the dispatch tree sees all three kinds)."""
    import torch

    from pgmpy_amd.program import Program

    E = _e()
    cases = [K.BY_NAME[n] for n in ("g8_ragged", "pair_gmid", "keep_order_new", "pair_rm2_elementwise", "ops8")]
    rng = np.random.default_rng(5)
    prog = Program()
    prog.begin_batch()
    items, gathers = [], []
    for i, c in enumerate(cases):
        arrays = K.make_values(c, "specials" if i % 2 else "signed")
        ops, buf, view = K.make_tensors(c, arrays, "cuda")
        items.append((c, arrays, buf, _record(prog, c, ops, view)))
        if i in (1, 3):  # a gather between the contractions
            g = K.GATHERS[len(gathers)]
            a = rng.uniform(-1.0, 1.0, [g["ext"][l] for l in g["la"]])
            A = E.to_device(a)
            codes, n_rows, ld = None, g["n_rows"], 0
            ev = {l: (None, v[1]) if isinstance(v, tuple) else v for l, v in g["evidence"].items()}
            if n_rows:
                ld = n_rows + 11
                hc = np.full((2, ld), 251, dtype=np.uint8)
                hc[1, 5:5 + n_rows] = rng.integers(0, g["ext"]["y"], n_rows)
                codes = E.to_device_raw(hc)
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            out = prog.gather(A, list(g["la"]), ev, [E.ROW if l == "R" else l for l in g["out"]], codes, ld, 5 if n_rows else 0,
                              n_rows, err)
            gathers.append((g, a, None if codes is None else hc[1, 5:5 + n_rows].astype(int), out, err))
    prog.end_batch()
    assert prog.check_hazards() == []
    prog.run()
    torch.cuda.synchronize()
    assert prog.notes == ["specialised batch of 7"], prog.notes
    src = _source(prog._pm_bound[0])
    assert src.count("(const unsigned char *)a.p[") == 2 and "lane_g" in src and "double lo = " in src
    worst = 0.0
    for c, arrays, buf, out in items:
        worst = max(worst, K.compare(c, out.cpu().numpy(), arrays))
        if c["out_kind"] == "pad":
            K.check_sentinels(c, buf.cpu().numpy())
    print(f"mixed level: worst |got - ref| / bound = {worst:.3f}")
    (g0, a0, _, o0, e0), (g1, a1, y, o1, e1) = gathers
    np.testing.assert_array_equal(o0.cpu().numpy(), a0[2].T)  # [s, a, k] at s = 2 -> [k, a]
    np.testing.assert_array_equal(o1.cpu().numpy(), np.moveaxis(a1[y], 0, 1))  # [row, a, k] -> [a, row, k]
    assert int(e0.item()) == 0 and int(e1.item()) == 0


# ----------------------------------------------------------------------------- single-workgroup chains
class Chain:
    """A chain of tiny dependent levels of nary_cases.CHAINS as a plain Program."""

    def __init__(self, name):
        import torch

        from pgmpy_amd.program import Program

        self.ext, self.levels = K.CHAINS[name]
        self.prog = Program()
        self.jobs = {}  # name -> (job, case, fresh input views by operand index, output buffer, output)
        for level in self.levels:
            self.prog.begin_batch()
            for j in level:
                c = K.chain_case(self.ext, j)
                ops, fresh = [], {}
                for t, (src, ls, view) in enumerate(j["ops"]):
                    if src is None:
                        shape = [self.ext[l] for l in ls]
                        n, off, st = K.operand_layout(shape, view)
                        v = torch.as_strided(torch.zeros(n, dtype=torch.float64, device="cuda"), shape, st, off)
                        fresh[t] = v
                    else:
                        have = self.jobs[src][0]["out"]
                        assert sorted(have) == sorted(ls)
                        v = self.jobs[src][4].permute([have.index(l) for l in ls]) if ls else self.jobs[src][4]
                    ops.append(v)
                buf = view = None
                lay = K.out_layout(K.out_shape(c), j["out_kind"])
                if lay is not None:
                    buf = torch.full((lay[0],), K.SENTINEL, dtype=torch.float64, device="cuda")
                    view = torch.as_strided(buf, K.out_shape(c), lay[2], lay[1])
                self.jobs[j["name"]] = (j, c, fresh, buf, _record(self.prog, c, ops, view))
            self.prog.end_batch()
        assert self.prog.check_hazards() == []

    def set(self, values):
        import torch

        self.inputs = {}
        for name, (j, c, fresh, buf, out) in self.jobs.items():
            arrays = K.make_values(c, values if len(fresh) == len(j["ops"]) else "signed")
            self.inputs[name] = arrays
            for t, v in fresh.items():
                v.copy_(torch.from_numpy(arrays[t]).reshape(list(v.shape)))
        self.clear()

    def clear(self):
        for j, c, fresh, buf, out in self.jobs.values():
            (out if buf is None else buf).fill_(K.SENTINEL)

    def results(self):
        import torch

        torch.cuda.synchronize()
        return {name: x[4].cpu().numpy() for name, x in self.jobs.items()}

    def check(self, got, what):
        """Every level's outputs, each against the reference on the inputs it actually read (the device's own
        outputs of the earlier levels)."""
        worst = 0.0
        for name, (j, c, fresh, buf, out) in self.jobs.items():
            arrays = []
            for t, (src, ls, view) in enumerate(j["ops"]):
                if src is None:
                    arrays.append(self.inputs[name][t])
                else:
                    have = self.jobs[src][0]["out"]
                    arrays.append(np.transpose(got[src], [have.index(l) for l in ls]) if ls else got[src])
            worst = max(worst, K.compare(c, got[name], arrays))
            if j["out_kind"] == "pad":
                K.check_sentinels(dict(c, out_kind="pad"), buf.cpu().numpy())
        print(f"{what}: {len(self.jobs)} jobs in {len(self.levels)} levels, worst |got - ref| / bound = {worst:.3f}")


_CHAINS = {}


def _chain(name):
    if name not in _CHAINS:
        _CHAINS[name] = Chain(name)
    return _CHAINS[name]


@pytest.mark.parametrize("name", sorted(K.CHAINS))
def test_single_workgroup_chain_matches_reference_at_every_level(gpu, name):
    """Dependent levels of tiny jobs lowered as one single-workgroup kernel: a level of more than 4 blocks, a
    consumer that reads its producer under a permuted label order, a producer written through a strided out=,
    n-ary and pair jobs in one level; every level's output is compared."""
    ch = _chain(name)
    n_levels = len(ch.levels)
    for values in ("signed", "specials"):
        ch.set(values)
        ch.prog.run()
        ch.check(ch.results(), f"chain {name}, {values}")
    assert len(ch.prog.notes) == 1 and ch.prog.notes[0].startswith(f"{n_levels} levels in one workgroup"), ch.prog.notes
    src = _source(ch.prog._pm_bound[0])
    assert src.count("__syncthreads();") == n_levels and "__launch_bounds__(1024)" in src
    if name == "nary_only":
        assert "for (unsigned b = 0u + vb; b < 7u; b += 4u)" in src  # the first level: 7 blocks, two rounds of four


# ----------------------------------------------------------------------------- the same bits in every form
def _forms(target, what):
    """target (a Level or a Chain, values set): its outputs after an eager run, a graph replay and a direct
    dispatch are bit-identical."""
    from pgmpy_amd.inference.plan import DirectQueue

    prog = target.prog
    assert prog._graph is None
    prog.run()
    eager = target.results()
    target.clear()
    prog.capture()
    assert prog._graph is not None
    prog.run()
    graph = target.results()
    target.clear()
    assert prog.bind_direct(DirectQueue()), prog.direct_note
    prog.run_direct()
    direct = target.results()
    names = eager.keys() if isinstance(eager, dict) else range(len(eager))
    for k in names:
        np.testing.assert_array_equal(_bits(eager[k]), _bits(graph[k]), err_msg=f"{what} {k}: graph")
        np.testing.assert_array_equal(_bits(eager[k]), _bits(direct[k]), err_msg=f"{what} {k}: direct")
    return eager


def test_level_batch_same_bits_eager_graph_direct(gpu):
    lv = Level(NAMED[-1])
    lv.set("specials")
    lv.check(_forms(lv, "level"), "level batch in three forms")


@pytest.mark.parametrize("name", sorted(K.CHAINS))
def test_chain_same_bits_eager_graph_direct(gpu, name):
    ch = Chain(name)
    ch.set("specials")
    ch.check(_forms(ch, f"chain {name}"), f"chain {name} in three forms")


SOLO = [c["name"] for c in K.CASES if K.prod(K.out_shape(c)) <= 5000]
SOLO_PARTS = _chunks(SOLO, 10)


@pytest.mark.parametrize("part", range(len(SOLO_PARTS)))
def test_job_alone_gives_the_bits_it_gives_in_its_batch(gpu, part):
    """A job's code and the order of its additions are its own: alone in a batch of one (same operands, an
    output of the same layout) it gives the bits it gives among the other jobs of its level batch."""
    import torch

    from pgmpy_amd.program import Program

    where = {c["name"]: (b, j) for b in range(len(NAMED)) for j, c in enumerate(NAMED[b])}
    t0 = time.perf_counter()
    together = {}
    for name in SOLO_PARTS[part]:
        b, j = where[name]
        lv = _level(("named", b), NAMED[b])
        if b not in together:
            together[b] = lv.run("specials")
        c, ops, buf, out = lv.items[j]
        view = None
        lay = K.out_layout(K.out_shape(c), c["out_kind"])
        if lay is not None:
            view = torch.as_strided(torch.full((lay[0],), K.SENTINEL, dtype=torch.float64, device="cuda"),
                                    K.out_shape(c), lay[2], lay[1])
        alone = Program()
        alone.begin_batch()
        o = _record(alone, c, ops, view)
        alone.end_batch()
        alone.run()
        torch.cuda.synchronize()
        assert alone.notes == ["specialised batch of 1"], alone.notes
        np.testing.assert_array_equal(_bits(o.cpu().numpy()), _bits(together[b][j]), err_msg=name)
    print(f"{len(SOLO_PARTS[part])} single-job kernels in {time.perf_counter() - t0:.2f} s")
