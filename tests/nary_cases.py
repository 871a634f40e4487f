"""Case table of the specialised batch generator (pgmi_cs_bind: one hipRTC kernel per level batch, emitted by
cs_nary_body / cs_job_body / cs_gather_body).  A plain module shared by tests/test_nary_cases_cpu.py (the plan
of every entry, no device) and tests/test_nary_paths_gpu.py (every entry run on the GPU).

An n-ary job is C[out] = REDUCE over the other labels of X_0 * X_1 * ... (a left fold, every product rounded
to fp64 before it is summed).  plan_contract_n drops unit dims, merges adjacent dims that every operand (and C)
steps through as one, and gives an output G = 2^g_log2 lanes while n_out * G < 16384 and 2G <= n_red; the
generator then picks, with P = 64 / G:

  nr == 0            a pure product
  G == 1             literal nested loops over the reduction, unrolled while the inner trip product is <= 64
  1 < G < 64         out = (tid >> 6) * P + (tid & (P - 1)), lane_g = (tid & 63) / P, shuffles 32 .. P
  G == 64            lane_g = tid & 63, shuffles 32 .. 1
  sd < nr            the lanes stride over the first sd reduced dims (the fewest whose product reaches G), the
                     dims [sd, nr) are literal loops (unrolled while their product is <= 64)
  sd == nr           the whole reduction index flattened and decoded per entry

`plan_nary` and `plan_pair` restate those decisions in plain Python; `classes_*` name the paths a plan takes.
Every named case lists the classes it exists for in `want`; the CPU test checks them against the library's own
plan (pgm_contract_n_info / pgm_contract_info), so a planner change that moves a case off its path fails there.

Labels are single characters with extents in `ext`.  An operand is (labels, view): "c" a C-order array, "T" a
transposed view (the buffer is C-order over the reversed labels), "s2" every other element along the last
axis, "off" a C-order array one element into its buffer (address 8 mod 16), "s2off" both.  `out_kind`: None
(the C-order output the engine allocates), "T" (a transposed view) or "pad" (a slice of a larger
sentinel-filled buffer: PAD_LO / PAD_HI extra elements around every axis, every other element of a 1-D buffer,
one element of four for a scalar).
"""
import math

import numpy as np

LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 2.0 ** -60  # 80-bit extended or better; else math.fsum of the fp64 terms
SENTINEL = -12345.678
DENORMAL = 5e-324 * 1023
PAD_LO, PAD_HI = 1, 2

NARY_LANES = 16384  # plan_contract_n: lanes of one job up to which an output gets more lanes
PAIR_LANES = 4096  # pgm_batch_add_contract, grid mode (256 in the single-workgroup chain)
UNROLL_PROD = 64  # inner trip product up to which reduction loops are fully unrolled
MAX_BLOCKS, MAX_BLOCKS_PRODUCT = 256, 1024  # 256-thread blocks one job takes (with / without a reduction)
MAX_RED = 4096
MAX_WORK = 1 << 21  # outputs x reduction entries of any case (the reference holds every term)

VIEWS = ("c", "T", "s2", "off", "s2off")


def prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


def c_strides(shape):
    st, acc = [], 1
    for c in reversed(list(shape)):
        st.append(acc)
        acc *= int(c)
    return st[::-1]


def operand_layout(shape, view):
    """(buffer elements, offset, strides) of an operand view, in elements."""
    shape = list(shape)
    n = prod(shape)
    if not shape:
        return (2, 1, []) if view in ("off", "s2off") else (1, 0, [])
    if view == "c":
        return n, 0, c_strides(shape)
    if view == "T":
        return n, 0, c_strides(shape[::-1])[::-1]
    if view == "off":
        return n + 1, 1, c_strides(shape)
    big = shape[:-1] + [2 * shape[-1]]
    st = c_strides(big)
    st[-1] = 2
    if view == "s2":
        return prod(big), 0, st
    assert view == "s2off", view
    return prod(big), 1, st


def out_layout(shape, kind):
    """(buffer elements, offset, strides) of the output view; None for the engine's own C-order output."""
    shape = list(shape)
    if kind is None:
        return None
    if kind == "T":
        return prod(shape), 0, c_strides(shape[::-1])[::-1]
    assert kind == "pad", kind
    if not shape:
        return 4, 1, []
    if len(shape) == 1:
        return 2 * shape[0] + PAD_LO + PAD_HI, PAD_LO, [2]
    buf = [s + PAD_LO + PAD_HI for s in shape]
    st = c_strides(buf)
    return prod(buf), sum(PAD_LO * s for s in st), st


def view_offsets(shape, off, strides):
    """Flat buffer index of every element of a view, in the view's C order."""
    idx = np.full((), int(off), dtype=np.int64)
    for n, s in zip(shape, strides):
        idx = idx[..., None] + np.arange(int(n), dtype=np.int64) * int(s)
    return idx.reshape([int(n) for n in shape])


# ----------------------------------------------------------------------------- cases
def nary(name, ext, ops, out, reduce="sum", views=None, out_kind=None, expect=None, want=()):
    ops = [list(o) for o in ops]
    views = list(views) if views is not None else ["c"] * len(ops)
    assert len(views) == len(ops) and all(v in VIEWS for v in views)
    return dict(kind="nary", name=name, ext=dict(ext), ops=ops, views=views, out=list(out), reduce=reduce,
                out_kind=out_kind, expect=dict(expect or {}), want=set(want))


def pair(name, ext, la, lb, out, reduce, combine, views=("c", "c"), out_kind=None, want=()):
    ops = [list(la)] + ([] if lb is None else [list(lb)])
    assert (lb is None) == (combine == "copy")
    return dict(kind="pair", name=name, ext=dict(ext), ops=ops, views=list(views)[:len(ops)], out=list(out),
                reduce=reduce, combine=combine, out_kind=out_kind, expect={}, want=set(want))


def labels_of(c):
    return list(dict.fromkeys(l for o in c["ops"] for l in o))


def red_labels(c):
    return [l for l in labels_of(c) if l not in c["out"]]


def op_shape(c, t):
    return [c["ext"][l] for l in c["ops"][t]]


def out_shape(c):
    return [c["ext"][l] for l in c["out"]]


def n_red_of(c):
    return prod(c["ext"][l] for l in red_labels(c))


def _stride_of(c, t, l):
    ls = c["ops"][t]
    if l not in ls:
        return 0
    return operand_layout(op_shape(c, t), c["views"][t])[2][ls.index(l)]


def _out_strides(c):
    lay = out_layout(out_shape(c), c["out_kind"])
    return c_strides(out_shape(c)) if lay is None else lay[2]


# ----------------------------------------------------------------------------- the plans, restated
def _collect(cards, strides):
    """Unit dims dropped, a dim merged into the previous (outer) one when every stride list steps through the two
    as one.  strides: one list per operand (and C).  Returns (cards, strides per operand)."""
    oc, os_ = [], [[] for _ in strides]
    for i, card in enumerate(cards):
        if card == 1:
            continue
        if oc and all(s_o[-1] == s[i] * card for s_o, s in zip(os_, strides)):
            oc[-1] *= card
            for s_o, s in zip(os_, strides):
                s_o[-1] = s[i]
            continue
        oc.append(card)
        for s_o, s in zip(os_, strides):
            s_o.append(s[i])
    return oc, os_


def plan_nary(c):
    """plan_contract_n and cs_nary_body's choices for an n-ary case."""
    n = len(c["ops"])
    keep, red = c["out"], red_labels(c)
    ksc = _out_strides(c)
    kc, ks = _collect([c["ext"][l] for l in keep], [ksc] + [[_stride_of(c, t, l) for l in keep] for t in range(n)])
    rc, rs = _collect([c["ext"][l] for l in red], [[_stride_of(c, t, l) for l in red] for t in range(n)])
    n_out, n_red = prod(kc), prod(rc)
    g = 0
    if rc:
        while g < 6 and (n_out << g) < NARY_LANES and (1 << (g + 1)) <= n_red:
            g += 1
    G = 1 << g
    blocks = min(max(((n_out << g) + 255) // 256, 1), MAX_BLOCKS if rc else MAX_BLOCKS_PRODUCT)
    sd, inner = len(rc), n_red
    if G > 1:
        p = 1
        for i, card in enumerate(rc):
            p *= card
            if p >= G:
                sd = i + 1
                break
        if sd >= len(rc):
            sd = len(rc)
        inner = prod(rc[sd:])
    # the literal loops' unroll boundary: dims [first_unrolled, nr) are fully unrolled
    lo = sd if G > 1 else 0
    first_unrolled, p = len(rc), 1
    for r in range(len(rc) - 1, lo - 1, -1):
        p *= rc[r]
        if p > UNROLL_PROD:
            break
        first_unrolled = r
    return dict(nk=len(kc), nr=len(rc), kcard=kc, rcard=rc, ksc=ks[0], ks=ks[1:], rs=rs, n_out=n_out, n_red=n_red,
                g_log2=g, G=G, P=64 // G, blocks=blocks, sd=sd, inner=inner, first_unrolled=first_unrolled,
                rolled=first_unrolled > lo)


def classes_nary(c, p=None):
    """Names of the generator paths and layout features an n-ary case reaches."""
    p = p or plan_nary(c)
    G, P, nr, n_out = p["G"], p["P"], p["nr"], p["n_out"]
    s = {f"ops{len(c['ops'])}", c["reduce"]}
    if nr == 0:
        s.add("nr0")
        if n_out > p["blocks"] * 256:
            s.add("grid_stride_product")
    else:
        if n_out * G > p["blocks"] * 256:
            s.add("grid_stride")
        if G == 1:
            s |= {"g1", "g1_rolled" if p["rolled"] else "g1_unrolled"}
        else:
            s.add(f"g{G}")
            if G < 64:
                if n_out > P and n_out % P:
                    s.add(f"g{G}_ragged")
                if n_out < P:
                    s.add(f"g{G}_below_p")
                if n_out == 1 and p["nk"] == 0:
                    s.add(f"g{G}_scalar")
            if p["sd"] < nr:
                s |= {"split", "split_inner_rolled" if p["rolled"] else "split_inner_unrolled"}
            else:
                s.add("flat_decode")
            if nr in (3, 4):
                s.add("sd%s_of_many" % ("nr" if p["sd"] == nr else p["sd"]))
    desc = lambda xs: all(a > b for a, b in zip(xs, xs[1:]))  # noqa: E731
    if p["nk"] >= 2:
        if not desc(p["ksc"]):
            s.add("ksc_not_monotone")
        multi = [[x for x in ks if x] for ks in p["ks"]]
        multi = [m for m in multi if len(m) >= 2]
        if multi and not any(desc(m) for m in multi):
            s.add("keep_order_new")
    if any(x == 0 for ks in p["ks"] for x in ks):
        s.add("kept_stride0")
    if any(c["ext"][l] == 1 for l in c["out"]):
        s.add("card1_kept")
    if any(c["ext"][l] == 1 for l in red_labels(c)):
        s.add("card1_reduced")
    if p["nk"] < sum(1 for l in c["out"] if c["ext"][l] > 1):
        s.add("kept_merge")
    if p["nr"] < sum(1 for l in red_labels(c) if c["ext"][l] > 1):
        s.add("red_merge")
    for v in c["views"]:
        s.add("op_" + v)
    if c["out_kind"]:
        s.add("out_" + c["out_kind"])
    return s


def plan_pair(c, lanes_cap=PAIR_LANES, a_ptr=0, b_ptr=0, c_ptr=0):
    """plan_contract's coalescing, then pgm_batch_add_contract's flat-mode plan (lanes per output, output pairs)
    and cs_red_loops_open's unroll boundary, for a pair case."""
    keep, red = c["out"], red_labels(c)
    use_b = len(c["ops"]) > 1
    sa = lambda ls: [_stride_of(c, 0, l) for l in ls]  # noqa: E731
    sb = lambda ls: [_stride_of(c, 1, l) if use_b else 0 for l in ls]  # noqa: E731
    kc, (ksa, ksb, ksc) = _collect([c["ext"][l] for l in keep], [sa(keep), sb(keep), _out_strides(c)])
    rc, (rsa, rsb) = _collect([c["ext"][l] for l in red], [sa(red), sb(red)])
    n_out, n_red = prod(kc), prod(rc)
    ri = rc[-1] if rc else 1
    n_ro = n_red // ri
    g = 0
    if c["reduce"] is not None and red and n_ro * ri > 1:
        while g < 6 and (n_out << g) < lanes_cap and (1 << (g + 1)) <= ri:
            g += 1
    kx = len(kc) - 1
    pairs = g == 0 and kx >= 0 and kc[kx] % 2 == 0 and ksc[kx] == 1 and c_ptr % 16 == 0
    va = pairs and ksa[kx] != 0
    vb = pairs and use_b and ksb[kx] != 0
    pairs = pairs and ksa[kx] in (0, 1) and (not use_b or ksb[kx] in (0, 1))
    for i in range(max(kx, 0)):
        pairs = pairs and ksc[i] % 2 == 0 and (not va or ksa[i] % 2 == 0) and (not vb or ksb[i] % 2 == 0)
    for i in range(len(rc) - 1):
        pairs = pairs and (not va or rsa[i] % 2 == 0) and (not vb or rsb[i] % 2 == 0)
    if pairs:
        ri_sa, ri_sb = (rsa[-1], rsb[-1]) if rc else (0, 0)
        pairs = (not va or (ri_sa % 2 == 0 and a_ptr % 16 == 0)) and (not vb or (ri_sb % 2 == 0 and b_ptr % 16 == 0))
    G = 1 << g
    trip = ri if (pairs or G == 1) else (ri + G - 1) // G
    first_unrolled, p = len(rc) - 1, trip
    for r in range(len(rc) - 2, -1, -1):
        p *= rc[r]
        if p > UNROLL_PROD:
            break
        first_unrolled = r
    return dict(nk=len(kc), nr=len(rc), kcard=kc, rcard=rc, n_out=n_out, n_red=n_red, n_ro=n_ro, ri_card=ri,
                g_log2=g, G=G, row_mode=2 if pairs else 0, va=bool(pairs and va), vb=bool(pairs and vb),
                outer_loops=max(len(rc) - 1, 0), rolled=len(rc) >= 2 and first_unrolled > 0)


def classes_pair(c, p):
    s = {"pair_%s_%s" % (c["combine"], c["reduce"] or "none")}
    if p["row_mode"] == 2:
        s.add("pair_rm2_va%d_vb%d" % (p["va"], p["vb"]))
    else:
        s.add("pair_g1" if p["G"] == 1 else "pair_g64" if p["G"] == 64 else "pair_gmid")
    if p["outer_loops"]:
        s.add("pair_outer_rolled" if p["rolled"] else "pair_outer_unrolled")
    for v in c["views"]:
        s.add("op_" + v)
    if c["out_kind"]:
        s.add("out_" + c["out_kind"])
    return s


def pair_ptrs(c):
    """Stand-in addresses with the alignment the views of a pair case get on the device (fresh buffers are 16-B
    aligned)."""
    base = 1 << 20
    a = base + 8 * operand_layout(op_shape(c, 0), c["views"][0])[1]
    b = base + 8 * operand_layout(op_shape(c, 1), c["views"][1])[1] if len(c["ops"]) > 1 else 0
    lay = out_layout(out_shape(c), c["out_kind"])
    return a, b, base + (8 * lay[1] if lay else 0)


def classes_of(c):
    if c["kind"] == "nary":
        return classes_nary(c)
    a, b, cp = pair_ptrs(c)
    return classes_pair(c, plan_pair(c, a_ptr=a, b_ptr=b, c_ptr=cp))


# the n-ary classes the issue lists; the table and the random family together must reach every one
NARY_CLASSES = (
    {"nr0", "g1_unrolled", "g1_rolled", "g64", "split_inner_unrolled", "split_inner_rolled", "flat_decode",
     "sd1_of_many", "sd2_of_many", "sdnr_of_many", "grid_stride", "grid_stride_product", "keep_order_new",
     "ksc_not_monotone", "kept_stride0", "card1_kept", "card1_reduced", "kept_merge", "out_pad", "out_T", "op_T",
     "op_s2", "op_off", "sum", "max"}
    | {f"g{G}{sfx}" for G in (2, 4, 8, 16, 32) for sfx in ("", "_ragged", "_below_p", "_scalar")}
    | {f"ops{n}" for n in range(1, 9)})
COMBINES = ("mul", "add", "div", "div_raw", "copy")
PAIR_CLASSES = (
    {"pair_rm2_va1_vb1", "pair_rm2_va1_vb0", "pair_rm2_va0_vb1"}
    | {"pair_g1", "pair_gmid", "pair_g64", "pair_outer_unrolled", "pair_outer_rolled"}
    | {"pair_%s_%s" % (cmb, r) for cmb in COMBINES for r in ("sum", "max", "none")})
# at least this many random n-ary cases in each of these
RANDOM_FLOOR = 10
RANDOM_FLOOR_CLASSES = ("nr0", "g1", "g2", "g4", "g8", "g16", "g32", "g64", "split", "flat_decode")


def _g_cases():
    """For every G in 2..32 (n_red in [G, 2G), n_out < 512): the plain lane map, an n_out that is no multiple of
    P, an n_out below P and the scalar output."""
    out = []
    for G, nred in ((2, 3), (4, 7), (8, 13), (16, 29), (32, 61)):
        P = 64 // G
        e = dict(g_log2=G.bit_length() - 1, n_red=nred)
        out.append(nary(f"g{G}_lanemap", dict(o=2 * P, r=nred), ["or", "r"], "o", expect=dict(e, n_out=2 * P),
                        want={f"g{G}", "flat_decode"}))
        out.append(nary(f"g{G}_ragged", dict(o=2 * P + 1 if P > 2 else 5, r=nred), ["or", "ro"], "o", "max",
                        expect=e, want={f"g{G}", f"g{G}_ragged"}))
        if P > 2:  # (G == 32: P == 2, the only n_out below P is the scalar output)
            out.append(nary(f"g{G}_below_p", dict(o=P - 1, r=nred), ["ro", "r"], "o", views=["T", "c"],
                            expect=dict(e, n_out=P - 1), want={f"g{G}_below_p"}))
        out.append(nary(f"g{G}_scalar", dict(r=nred), ["r", "r"], "", out_kind="pad" if G in (2, 32) else None,
                        expect=dict(e, n_out=1, nk=0), want={f"g{G}_scalar", f"g{G}_below_p"}))
    return out


CASES = [
    # ------------------------------------------------------------------ no reduction
    nary("nr0_outer", dict(i=5, j=7), ["i", "j"], "ji", expect=dict(nr=0, g_log2=0, n_out=35, blocks=1),
         want={"nr0", "ops2", "kept_stride0"}),
    nary("nr0_grid_stride", dict(i=513, j=513), ["i", "j"], "ij", expect=dict(nr=0, n_out=263169, blocks=1024),
         want={"nr0", "grid_stride_product"}),
    # ------------------------------------------------------------------ one lane per output (n_out >= 16384)
    nary("g1_unrolled", dict(o=16384, p=8, q=8), ["op", "pq", "q"], "o",
         expect=dict(g_log2=0, n_red=64, nr=2, blocks=64), want={"g1_unrolled", "ops3"}),
    nary("g1_rolled", dict(o=16385, p=5, q=13), ["op", "pq", "oq"], "o", "max",
         expect=dict(g_log2=0, n_red=65, nr=2, blocks=65), want={"g1_rolled", "max"}),
    nary("g1_grid_stride", dict(o=65537, r=2), ["or", "r"], "o", expect=dict(g_log2=0, n_out=65537, blocks=256),
         want={"g1_unrolled", "grid_stride"}),
    # ------------------------------------------------------------------ 1 < G < 64, G == 64
    *_g_cases(),
    nary("g64_ragged", dict(o=7, r=129), ["or", "r"], "o", expect=dict(g_log2=6, n_out=7, blocks=2),
         want={"g64", "flat_decode"}),
    nary("g64_scalar", dict(r=64), ["r"], "", "max", expect=dict(g_log2=6, nk=0, n_out=1), want={"g64", "ops1"}),
    # ------------------------------------------------------------------ outer / inner split of the reduction
    nary("split_inner_unrolled", dict(o=3, p=64, q=4, r=16), ["opq", "qr", "pr"], "o",
         expect=dict(g_log2=6, nr=3, rcard=[64, 4, 16]), want={"split_inner_unrolled", "sd1_of_many", "g64"}),
    nary("split_inner_rolled", dict(o=3, p=64, q=5, r=13), ["opq", "qr", "pr"], "o",
         expect=dict(g_log2=6, nr=3, rcard=[64, 5, 13]), want={"split_inner_rolled", "sd1_of_many"}),
    nary("split_sd2_of_4", dict(o=5, p=7, q=11, r=2, s=3), ["opq", "qrs", "ps"], "o", "max",
         expect=dict(g_log2=6, nr=4, rcard=[7, 11, 2, 3]), want={"sd2_of_many", "split_inner_unrolled"}),
    nary("split_sdnr_of_3", dict(o=5, p=3, q=2, r=7), ["opq", "qr", "pr"], "o",
         expect=dict(g_log2=5, nr=3, rcard=[3, 2, 7]), want={"sdnr_of_many", "flat_decode", "g32"}),
    nary("g16_many_blocks", dict(o=1100, r=64), ["or", "r"], "o", expect=dict(g_log2=4, blocks=69), want={"g16"}),
    # ------------------------------------------------------------------ kept dims
    nary("keep_order_new", dict(a=3, b=4, c=5, d=2), ["acb", "bd", "da"], "ca", out_kind="T",
         expect=dict(nk=2, kcard=[5, 3]), want={"keep_order_new", "ksc_not_monotone", "out_T", "kept_stride0"}),
    nary("card1_kept_and_reduced", dict(a=3, u=1, b=4, v=1, r=6), ["aub", "vr", "ru"], "uab",
         expect=dict(nk=1, nr=1, kcard=[12], rcard=[6]), want={"card1_kept", "card1_reduced", "kept_merge"}),
    nary("kept_merge", dict(a=4, b=6, r=5), ["abr", "r"], "ab", expect=dict(nk=1, kcard=[24], n_out=24),
         want={"kept_merge", "kept_stride0"}),
    nary("kept_no_merge_transposed", dict(a=4, b=6, r=5), ["abr", "ab"], "ab", views=["c", "T"],
         expect=dict(nk=2, kcard=[4, 6], n_out=24), want={"op_T"}),
    nary("red_merge", dict(o=3, p=4, q=5), ["opq", "pq"], "o", expect=dict(nr=1, rcard=[20]), want={"red_merge"}),
    # ------------------------------------------------------------------ strided out=, operand views
    nary("out_pad_2d", dict(a=5, b=7, r=9), ["ar", "rb"], "ab", out_kind="pad", expect=dict(nk=2, g_log2=3),
         want={"out_pad", "g8"}),
    nary("out_pad_1d", dict(a=37, r=3), ["ar", "r"], "a", "max", out_kind="pad", want={"out_pad", "g2"}),
    nary("out_T_product", dict(a=6, b=5), ["ab", "b"], "ab", out_kind="T", expect=dict(nr=0, nk=2),
         want={"nr0", "out_T"}),
    nary("views_mixed", dict(a=5, b=6, r=7), ["ar", "rb", "ab", "r"], "ab", views=["s2", "T", "off", "s2off"],
         want={"op_s2", "op_T", "op_off", "op_s2off", "ops4"}),
    # ------------------------------------------------------------------ operand counts
    nary("ops1_marginal", dict(a=6, r=10), ["ar"], "a", expect=dict(g_log2=3), want={"ops1"}),
    nary("ops5", dict(a=3, b=4, c=2), ["ab", "bc", "c", "a", "ca"], "a", want={"ops5"}),
    nary("ops6", dict(a=3, b=4, c=2), ["ab", "bc", "c", "a", "ca", "b"], "ca", "max", want={"ops6", "max"}),
    nary("ops7", dict(p=2, q=3), ["p"] * 6 + ["pq"], "q", want={"ops7"}),
    nary("ops8", dict(p=2, q=3), ["p"] * 7 + ["pq"], "q", views=["c", "off"] * 4, want={"ops8", "op_off"}),
    # ------------------------------------------------------------------ pair jobs: output pairs (row_mode 2)
    # (one lane per output is the choice only without a reduction or from 4096 outputs on; the innermost kept
    # label is in A or in B, so va and vb are never both off)
    pair("pair_rm2_va1_vb1", dict(a=700, x=6, r=5), "rax", "rx", "ax", "sum", "mul", want={"pair_rm2_va1_vb1"}),
    pair("pair_rm2_va1_vb0", dict(a=700, x=6, r=5), "rax", "ra", "ax", "max", "add", want={"pair_rm2_va1_vb0"}),
    pair("pair_rm2_va0_vb1", dict(a=700, x=6, r=5), "ra", "rax", "ax", "sum", "mul", want={"pair_rm2_va0_vb1"}),
    pair("pair_rm2_copy", dict(a=700, x=8, r=4), "rax", None, "ax", "sum", "copy", want={"pair_rm2_va1_vb0"}),
    pair("pair_rm2_elementwise", dict(a=3, x=8), "ax", "x", "ax", None, "div", want={"pair_rm2_va1_vb1"}),
    pair("pair_rm2_misaligned", dict(a=700, x=6, r=5), "rax", "rx", "ax", "sum", "mul", views=("off", "c"),
         want={"pair_g1", "op_off"}),
    # ------------------------------------------------------------------ pair jobs: flat mode
    pair("pair_g1_odd", dict(a=3, x=7), "ax", "x", "ax", None, "mul", want={"pair_g1", "pair_mul_none"}),
    pair("pair_gmid", dict(a=5, r=9), "ar", "r", "a", "sum", "mul", want={"pair_gmid"}),
    pair("pair_g64", dict(a=5, r=130), "ar", "r", "a", "max", "mul", want={"pair_g64", "pair_mul_max"}),
    pair("pair_outer_unrolled", dict(a=5, p=3, q=4, r=8), "apr", "qr", "a", "sum", "mul",
         want={"pair_outer_unrolled", "pair_gmid"}),
    pair("pair_outer_rolled", dict(a=5, p=9, q=8, r=8), "apr", "qr", "a", "sum", "mul",
         want={"pair_outer_rolled", "pair_gmid"}),
    pair("pair_outer_rolled_rm2", dict(a=1100, x=4, p=9, q=8, r=3), "prax", "qrx", "ax", "sum", "mul",
         want={"pair_outer_rolled", "pair_rm2_va1_vb1"}),
    pair("pair_out_pad", dict(a=5, b=3, r=9), "ar", "rb", "ba", "sum", "mul", out_kind="pad", want={"out_pad"}),
    pair("pair_views", dict(a=5, b=4, r=9), "ar", "rb", "ab", "sum", "div_raw", views=("T", "s2"),
         want={"op_T", "op_s2", "pair_div_raw_sum"}),
]
# every combine x every reduce pgm_batch_add_contract accepts
for _cmb in COMBINES:
    for _red in ("sum", "max", None):
        _lb = None if _cmb == "copy" else ("rb" if _red else "b")
        CASES.append(pair("pair_%s_%s" % (_cmb, _red or "none"), dict(a=3, b=5, r=4), "arb" if _red else "ab", _lb,
                          "ab", _red, _cmb, want={"pair_%s_%s" % (_cmb, _red or "none")}))

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ----------------------------------------------------------------------------- random families
def _random_labels(rng, n_keep, n_red, keep_cards, red_cards):
    names = "abcdefghijklmnopqrstuvwxyz"
    ext, keep, red = {}, [], []
    for i in range(n_keep + n_red):
        l = names[i]
        lo, hi = keep_cards if i < n_keep else red_cards
        ext[l] = int(rng.integers(lo, hi + 1))
        (keep if i < n_keep else red).append(l)
    return ext, keep, red


_TARGETS = {  # (kept labels, reduced labels, kept extents, reduced extents)
    "any": ((0, 4), (0, 3), (1, 9), (1, 9)),
    "nr0": ((1, 5), (0, 0), (1, 9), (1, 9)),
    "g1": ((5, 6), (1, 2), (5, 9), (2, 4)),
    "g2": ((0, 3), (1, 1), (1, 9), (2, 3)),
    "g4": ((0, 3), (1, 2), (1, 9), (2, 3)),
    "g8": ((0, 3), (1, 2), (1, 8), (2, 4)),
    "g16": ((0, 3), (2, 2), (1, 6), (4, 5)),
    "g32": ((0, 2), (2, 3), (1, 6), (3, 4)),
    "g64": ((0, 2), (2, 4), (1, 6), (3, 9)),
}


def _random_nary(rng, target, name):
    (k0, k1), (r0, r1), kc, rc = _TARGETS[target]
    ext, keep, red = _random_labels(rng, int(rng.integers(k0, k1 + 1)), int(rng.integers(r0, r1 + 1)), kc, rc)
    labels = keep + red
    if not labels:
        return None
    n_ops = int(rng.integers(1, 9))
    ops = []
    for _ in range(n_ops):
        k = int(rng.integers(1, min(5, len(labels)) + 1))
        ops.append([labels[i] for i in rng.permutation(len(labels))[:k]])
    for l in labels:  # every label in some operand with room for it
        if not any(l in o for o in ops):
            room = [o for o in ops if len(o) < 5]
            if not room:
                return None
            o = room[int(rng.integers(len(room)))]
            o.insert(int(rng.integers(len(o) + 1)), l)
    out = [keep[i] for i in rng.permutation(len(keep))]
    n_out, n_red = prod(ext[l] for l in keep), prod(ext[l] for l in red)
    if n_red > MAX_RED or n_out * n_red > MAX_WORK:
        return None
    views = [VIEWS[int(rng.integers(len(VIEWS)))] if rng.random() < 0.5 else "c" for _ in ops]
    out_kind = (None, None, "T", "pad")[int(rng.integers(4))]
    c = nary(name, ext, ops, out, "max" if rng.random() < 0.3 else "sum", views, out_kind)
    lay = out_layout(out_shape(c), out_kind)
    if max([lay[0] if lay else n_out] + [operand_layout(op_shape(c, t), views[t])[0] for t in range(n_ops)]) > 1 << 18:
        return None  # every tensor at most 2 MB
    return c


def random_cases(seed, n):
    """n seeded random n-ary cases: 1-8 operands of 1-5 labels, extents 1-9, a random output label order and
    random views; the shapes are drawn per target class in turn so every lane map keeps turning up."""
    rng = np.random.default_rng(seed)
    targets = list(_TARGETS)
    out = []
    while len(out) < n:
        c = _random_nary(rng, targets[len(out) % len(targets)], "rand%d_%d" % (seed, len(out)))
        if c is not None:
            out.append(c)
    return out


def random_pair_cases(seed, n):
    """n seeded random pair jobs: operands of 1-4 labels (the second absent for copy), extents 1-9 with an
    occasional long reduced label, every combine and reduce, random views and output order."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        ext, keep, red = _random_labels(rng, int(rng.integers(1, 4)), int(rng.integers(0, 3)), (1, 9), (1, 9))
        if red and rng.random() < 0.3:
            ext[red[-1]] = int(rng.integers(60, 140))
        if rng.random() < 0.4:
            ext[keep[-1]] = 2 * int(rng.integers(1, 5))
        labels = keep + red
        cmb = COMBINES[int(rng.integers(len(COMBINES)))]
        reduce = None if not red else ("sum", "max")[int(rng.integers(2))]
        la = [labels[i] for i in rng.permutation(len(labels))[:int(rng.integers(1, min(4, len(labels)) + 1))]]
        lb = None
        if cmb != "copy":
            lb = [labels[i] for i in rng.permutation(len(labels))[:int(rng.integers(1, min(4, len(labels)) + 1))]]
        have = set(la) | set(lb or [])
        if any(l not in have for l in labels):
            continue
        if rng.random() < 0.5:  # the layout that allows output pairs: kept labels in output order, the last innermost
            order = [l for l in red + keep]
            la = [l for l in order if l in la]
            lb = None if lb is None else [l for l in order if l in lb]
            okeep = list(keep)
        else:
            okeep = [keep[i] for i in rng.permutation(len(keep))]
        views = [VIEWS[int(rng.integers(len(VIEWS)))] if rng.random() < 0.3 else "c" for _ in range(2)]
        out.append(pair("randpair%d_%d" % (seed, len(out)), ext, la, lb, okeep, reduce, cmb, views,
                        (None, None, None, "T", "pad")[int(rng.integers(5))]))
    return out


RANDOM_SEEDS = (11, 12)  # 2 x 110 n-ary jobs
RANDOM_PER_SEED = 110
RANDOM_PAIR_SEED, RANDOM_PAIRS = 21, 110


def all_random():
    return [c for s in RANDOM_SEEDS for c in random_cases(s, RANDOM_PER_SEED)]


# ----------------------------------------------------------------------------- values
def _rng_for(c, salt):
    return np.random.default_rng([salt] + [ord(ch) for ch in c["name"]])


def _full_index(c, out_i, where):
    """label -> index of output `out_i` (modulo the output count) at the first / a middle / the last entry of
    the flattened reduction."""
    idx = {}
    oshape = out_shape(c)
    n_keep = prod(oshape)
    for l, v in zip(c["out"], np.unravel_index(out_i % n_keep, oshape) if oshape else ()):
        idx[l] = int(v)
    for l in red_labels(c):
        n = c["ext"][l]
        idx[l] = {"first": 0, "last": n - 1, "mid": n // 2}[where]
    return idx


def plant_specials(c, arrays):
    """NaN, +inf, -inf, -0.0 and a denormal at the first, a middle and the last reduction entry of fixed outputs
    (the last entry falls in the last lane of the last ragged round), and one output whose whole reduction is
    -inf, written into the operand with the most labels (an operand that lacks a label spreads the value over
    that label; the reference sees the same arrays).  Without a reduction the entries are plain elements."""
    t = max(range(len(arrays)), key=lambda i: (arrays[i].ndim, -i))
    a, ls = arrays[t], c["ops"][t]
    n_keep = prod(out_shape(c))
    if a.ndim == 0:
        return arrays
    plants = [(0, "first", np.nan), (1, "last", np.nan), (3, "last", np.inf), (4, "first", np.inf),
              (4, "last", -np.inf), (5, "first", -np.inf), (6, "mid", -0.0), (6, "last", DENORMAL),
              (n_keep - 1, "mid", np.nan)][:9 if n_keep > 8 else 8]
    if n_keep > 2:
        idx = _full_index(c, 2, "first")
        a[tuple(idx[l] if l in c["out"] else slice(None) for l in ls)] = -np.inf
    for out_i, where, v in plants:
        if out_i < n_keep and not (out_i == 2 and n_keep > 2):
            idx = _full_index(c, out_i, where)
            a[tuple(idx[l] for l in ls)] = v
    return arrays


def make_values(c, values):
    """One fp64 array per operand (its logical shape): "signed" uniform in [-1, 1], "zeros" the same with whole
    slices of exact zeros in every other operand, "specials" with plant_specials.  Divisors keep away from 0."""
    rng = _rng_for(c, {"signed": 1, "zeros": 2, "specials": 3}[values])
    arrays = [rng.uniform(-1.0, 1.0, op_shape(c, t)) for t in range(len(c["ops"]))]
    if c["kind"] == "pair" and c["combine"] in ("div", "div_raw") and len(arrays) > 1:
        arrays[1] = rng.uniform(0.5, 1.5, arrays[1].shape) * rng.choice([-1.0, 1.0], arrays[1].shape)
    if values == "zeros":
        for t, a in enumerate(arrays):
            if (t % 2 == 0 or len(arrays) == 1) and a.ndim:
                ax = int(np.argmax(a.shape))
                sl = [slice(None)] * a.ndim
                sl[ax] = a.shape[ax] // 2
                a[tuple(sl)] = 0.0
    if values == "specials":
        plant_specials(c, arrays)
    return arrays


# ----------------------------------------------------------------------------- reference
def _bcast(c, x, labels, order):
    have = [l for l in order if l in labels]
    x = np.transpose(x, [labels.index(l) for l in have]) if x.ndim else x
    return x.reshape([c["ext"][l] if l in labels else 1 for l in order])


def terms(c, arrays):
    """Every term of every output, fp64, shape (n_out, n_red): the operands multiplied in order (a left fold,
    one rounding per product — the generator's contract), or the pair job's combine."""
    order = c["out"] + red_labels(c)
    full = [c["ext"][l] for l in order]
    with np.errstate(all="ignore"):
        if c["kind"] == "pair":
            a = _bcast(c, arrays[0], c["ops"][0], order)
            cmb = c["combine"]
            if cmb == "copy":
                t = a
            else:
                b = _bcast(c, arrays[1], c["ops"][1], order)
                t = a * b if cmb == "mul" else a + b if cmb == "add" else a / b
                if cmb == "div":
                    t = np.where(np.isnan(t), 0.0, t)
        else:
            t = _bcast(c, arrays[0], c["ops"][0], order)
            for x, ls in zip(arrays[1:], c["ops"][1:]):
                t = t * _bcast(c, x, ls, order)
        t = np.broadcast_to(t, full)
    return np.ascontiguousarray(t, dtype=np.float64).reshape(prod(out_shape(c)), -1)


def ref(c, arrays):
    """(reference, mag) over the output's shape.  Sum: the fp64 terms added in long double (math.fsum without
    one), mag = sum of |term| over the finite terms.  Max and no reduction: exact in fp64, mag None."""
    t = terms(c, arrays)
    shape = out_shape(c)
    with np.errstate(all="ignore"):
        if c["reduce"] == "sum":
            mag = np.where(np.isfinite(t), np.abs(t), 0.0).astype(LD).sum(axis=1)
            if HAVE_LD:
                r = t.astype(LD).sum(axis=1)
            else:
                r = np.array([math.fsum(row) if np.isfinite(row).all() else row.sum() for row in t]).astype(LD)
            return r.reshape(shape), mag.reshape(shape)
        if c["reduce"] == "max":
            return np.max(t, axis=1).reshape(shape), None
        assert t.shape[1] == 1, c["name"]
        return t[:, 0].reshape(shape), None


def bound(c, mag):
    """|got - ref| <= (n_red + 2) * 2^-53 * mag: n_red - 1 additions in any order, first order in 2^-53; the + 2
    covers the second-order terms and the rounding of the reference to fp64."""
    return (n_red_of(c) + 2) * LD(2.0) ** -53 * mag


def compare(c, got, arrays):
    """Assert got against ref(c, arrays) (the bound for sums, exactly otherwise, the NaN / inf pattern exactly,
    every output).  Returns the worst |got - ref| / bound (0.0 for exact cases)."""
    r, mag = ref(c, arrays)
    got = np.asarray(got)
    assert got.shape == r.shape, (c["name"], got.shape, r.shape)
    if mag is None:
        np.testing.assert_array_equal(got, r, err_msg=c["name"])
        return 0.0
    np.testing.assert_array_equal(np.isnan(got), np.isnan(r), err_msg=c["name"])
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(r), err_msg=c["name"])
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(r), err_msg=c["name"])
    fin = np.isfinite(r)
    err = np.abs(got[fin].astype(LD) - r[fin])
    b = bound(c, mag[fin])
    ratio = float(np.max(err / np.where(b > 0, b, 1), initial=0.0))
    bad = err > b
    assert not bad.any(), f"{c['name']}: {int(bad.sum())} outputs beyond the summation bound (worst ratio {ratio:.3f})"
    return ratio


# ----------------------------------------------------------------------------- gathers and chains
# evidence gathers mixed into a level (engine.prepare_gather): (labels of A, extents, evidence, output labels);
# evidence values: an int (static) or ("col", j) (the per-row code column j), "R" stands for the row label
GATHERS = [
    dict(name="gather_static", la="sak", ext=dict(s=3, a=4, k=5), evidence={"s": 2}, out="ka", n_rows=None),
    dict(name="gather_rows", la="yak", ext=dict(y=6, a=4, k=5), evidence={"y": ("col", 1)}, out="aRk", n_rows=37),
]


def job(name, ops, out, reduce="sum", combine=None, out_kind=None):
    """A chain job: ops are (source, labels, view); source None is a fresh input over `labels`, a job name is
    that job's output read with the axes permuted into `labels` order (labels: the producer's output labels in
    any order)."""
    return dict(name=name, ops=[(s, list(ls), v) for s, ls, v in ops], out=list(out), reduce=reduce,
                combine=combine, out_kind=out_kind)


# chains of tiny dependent levels, lowered as "levels in one workgroup"; each: (extents, levels of jobs)
CHAINS = {
    "nary_only": (dict(a=5, b=6, c=4, p=20, r=64, i=3, j=7, x=3), [
        [job("j0", [(None, "ab", "c"), (None, "bc", "T")], "ac"),
         job("j1", [(None, "pr", "c"), (None, "r", "off")], "p"),  # 20 outputs x 64 lanes: 5 blocks
         job("j2", [(None, "i", "c"), (None, "j", "c")], "ji", out_kind="pad")],
        [job("j3", [("j0", "ca", "c"), (None, "xca", "c")], "x"),  # j0 read under the permuted order [c, a]
         job("j4", [("j2", "ji", "c"), (None, "i", "s2")], "j", "max")],  # j2 was written through a padded view
        [job("j5", [("j3", "x", "c"), ("j1", "p", "c")], "p"),
         job("j6", [("j4", "j", "c")], "")],
    ]),
    "mixed": (dict(a=5, b=6, c=4, x=3, r=9), [
        [job("m0", [(None, "ab", "c"), (None, "bc", "c")], "ac", "sum", "mul"),
         job("m1", [(None, "ar", "c"), (None, "rc", "s2"), (None, "c", "c")], "ca")],
        [job("m2", [("m0", "ac", "c")], "a", "sum", "copy"),
         job("m3", [("m1", "ac", "c"), ("m0", "ac", "c"), (None, "xc", "c")], "xa", out_kind="pad")],
        [job("m4", [("m0", "ac", "c"), ("m2", "a", "c")], "ac", None, "div_raw"),
         job("m5", [("m3", "ax", "c"), ("m2", "a", "c")], "x", "max")],
        [job("m6", [("m4", "ca", "c"), ("m5", "x", "c")], "xc")],
    ]),
}


def chain_case(ext, j):
    """The chain job as a case of this module (for ref / compare): produced operands are C-order inputs here."""
    ops = [ls for _, ls, _ in j["ops"]]
    if j["combine"]:
        return pair(j["name"], ext, ops[0], ops[1] if len(ops) > 1 else None, j["out"], j["reduce"], j["combine"])
    return nary(j["name"], ext, ops, j["out"], j["reduce"])


# ----------------------------------------------------------------------------- tensors (torch imported on use)
def make_tensors(c, arrays, device):
    """(operand views, output buffer, output view) of a case on `device`: every operand a view with its kind's
    strides and offset into a flat buffer of its own, the output a view into a sentinel-filled buffer (None, None
    for the engine-allocated output)."""
    import torch

    ops = []
    for t, a in enumerate(arrays):
        shape = op_shape(c, t)
        n, off, st = operand_layout(shape, c["views"][t])
        buf = torch.zeros(n, dtype=torch.float64, device=device)
        v = torch.as_strided(buf, shape, st, off)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).reshape(shape))
        assert v.data_ptr() % 16 == (8 * off) % 16
        ops.append(v)
    lay = out_layout(out_shape(c), c["out_kind"])
    if lay is None:
        return ops, None, None
    buf = torch.full((lay[0],), SENTINEL, dtype=torch.float64, device=device)
    return ops, buf, torch.as_strided(buf, out_shape(c), lay[2], lay[1])


def set_values(c, ops, arrays):
    """New values into the operand views make_tensors made (same buffers, same descriptors)."""
    import torch

    for t, (v, a) in enumerate(zip(ops, arrays)):
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).reshape(op_shape(c, t)))


def check_sentinels(c, buf):
    """Nothing outside the output view of a strided out= was written (buf: the host copy of the buffer)."""
    lay = out_layout(out_shape(c), c["out_kind"])
    mask = np.ones(lay[0], dtype=bool)
    mask[view_offsets(out_shape(c), lay[1], lay[2]).reshape(-1)] = False
    assert (np.asarray(buf)[mask] == SENTINEL).all(), f"{c['name']}: an element outside the output view was overwritten"
