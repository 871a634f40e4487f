"""The pseudo-likelihood plan without a device (pgm_mnpl_plan_create / pgm_mnpl_plan_info, csrc/pgmmnpl_plan.cpp): the
blanket families, the part slots, the LDS limit, the argument checks; and that the random rows of the cases hold what
the GPU tests rely on."""
import ctypes

import numpy as np
import pytest

from pgmpy_amd import _native as N
from pgmpy_amd.estimators._mnpl import MnplPlan
from tests.mnpl_cases import CHAIN, LDS_PAD, TRIANGLE, blanket, cases, family_data, star_leaves

LDS_MAX = 163840 - 256
CASES = cases(LDS_MAX)


def plan_of(case):
    return MnplPlan([(list(s), [case["card"][v] for v in s]) for s in case["scopes"]], case["card"])


@pytest.mark.parametrize("name", list(CASES))
def test_blanket_families_and_slots(name):
    case = CASES[name]
    card, scopes = case["card"], case["scopes"]
    plan = plan_of(case)
    assert plan.info.lds_max == LDS_MAX and plan.info.block == 256
    want = [([i] + blanket(scopes, i), [card[v] for v in [i] + blanket(scopes, i)]) for i in range(len(card))]
    assert plan.families == want
    fit = plan.fit_plan()  # the fit plan lays the count tables out as the kernel reads them
    assert fit.offsets == plan.count_offsets[:-1] and fit.total_bins == plan.n_counts
    sizes = [int(np.prod([card[v] for v in s])) for s in scopes]
    assert plan.sizes == sizes and plan.n_theta == sum(sizes)
    # every (factor, member) exactly once, by node then factor; the slots tile the parts buffer
    assert [(f, m) for f, m, _ in plan.slots] == [(f, s.index(i)) for i in range(len(card))
                                                  for f, s in enumerate(scopes) if i in s]
    spans = sorted((off, off + sizes[f]) for f, _, off in plan.slots)
    assert spans[0][0] == 0 and spans[-1][1] == plan.n_parts == sum(len(s) * z for s, z in zip(scopes, sizes))
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    resid = [8 * int(np.prod(c)) + LDS_PAD for _, c in want]
    assert all(lds >= r for lds, r in zip(plan.node_lds, resid)) and plan.info.lds_bytes == max(plan.node_lds) <= LDS_MAX
    # the incident tables are staged wherever they fit: everywhere but in the case made so that they do not
    assert plan.info.theta_lds_nodes == (0 if name == "wide_theta" else len(card))


def test_largest_star_is_accepted_and_the_next_rejected():
    n = star_leaves(LDS_MAX)
    plan = plan_of(CASES["star"])
    assert (plan.info.max_node, plan.info.max_degree) == (0, n) and plan.node_lds[0] >= 16 * 2 ** n + LDS_PAD
    with pytest.raises(ValueError, match=rf"node 0 with {n + 1} blanket columns .* {16 * 2 ** (n + 1)} bytes"):
        MnplPlan([([0, j], [2, 2]) for j in range(1, n + 2)], [2] * (n + 2))
    with pytest.raises(ValueError, match=r"node 0 has 32 blanket columns \(31 at most\)"):
        MnplPlan([([0, j], [1, 1]) for j in range(1, 33)], [1] * 33)


def test_argument_checks_before_any_device_call():
    L = N.load_library()
    assert all(f"pgm_mnpl_{n}" in N.EXPORTED for n in ("plan_create", "plan_destroy", "plan_info", "eval"))
    with pytest.raises(ValueError, match="column 1 is in no factor"):
        MnplPlan([([0], [2])], [2, 2])
    with pytest.raises(ValueError, match="cardinality 3, the column has 2"):
        MnplPlan([([0, 1], [2, 3])], [2, 2])
    plan = plan_of(CASES["chain"])
    buf = np.zeros(64)
    p = lambda k=0: ctypes.c_void_p(buf.ctypes.data + k)
    for args, what in (((None, p(), p(), 0.0, p(), p(), p()), "null plan"), ((plan._h, None, p(), 0.0, p(), p(), p()), "null counts"),
                       ((plan._h, p(), p(), 0.0, None, p(), p()), "null value"), ((plan._h, p(), p(), -1.0, p(), p(), p()), "l2 -1"),
                       ((plan._h, p(), p(), float("nan"), p(), p(), p()), "l2 nan"),
                       ((plan._h, p(), p(4), 0.0, p(), p(), p()), "not 8-byte aligned")):
        assert L.pgm_mnpl_eval(*args, None) == N.PGM_EINVAL and what in N.last_error()


@pytest.mark.parametrize("card,scopes,codes", [(CASES[n]["card"], CASES[n]["scopes"], CASES[n]["codes"])
                                               for n in ("unary", "chain", "triangle")]
                         + [(*CHAIN, family_data(*CHAIN, 11)[0]), (*TRIANGLE, family_data(*TRIANGLE, 12)[0])])
def test_every_state_occurs_under_every_blanket_configuration(card, scopes, codes):
    """What stationarity needs (a finite optimum): on the small cases' random rows and on the fit test's data.  The
    grid's and the star's tables are mostly empty on purpose and no fit is run on them."""
    for i in range(len(card)):
        family = [i] + blanket(scopes, i)
        seen = {tuple(row) for row in codes[family].T}
        assert len(seen) == int(np.prod([card[v] for v in family]))


def test_public_interface_without_a_device():
    import torch

    from pgmpy_amd.estimators import PseudoLikelihoodEstimator
    from pgmpy_amd.models import DiscreteMarkovNetwork

    model = DiscreteMarkovNetwork([("b", "a"), ("b", "c")])
    model.add_node("d")
    with pytest.raises(ValueError, match="not supported"):
        model.fit(None, estimator="mle")
    assert PseudoLikelihoodEstimator(model)._scopes == [("a", "b"), ("b", "c"), ("d",)]  # an edge each, the isolated node
    if not torch.cuda.is_available():
        with pytest.raises(N.NativeUnavailable):
            model.fit_codes(torch.zeros((4, 8), dtype=torch.uint8))
