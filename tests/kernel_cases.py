"""Case table of the pgm_contract kernel paths (a plain module: tests/test_kernel_plan_cpu.py checks the
plan of every entry without a device, tests/test_kernel_paths_gpu.py runs every entry on the GPU).

pgm_contract dispatches to k_contract (flat: G lanes per output, optional split-K), k_contract_rows
(innermost kept dim across lanes; the 4-wide elementwise loop; split over (reduction-outer, chunk of the
innermost reduction dim)), k_contract_rows_tab / _tab2 (<= 512 reduction offsets in LDS) and, after a
split, k_contract_final.  Each entry names the path it exists for and records the plan fields
(pgm_contract_info) that prove a shape takes it; a planner change that moves a shape to another path fails
the CPU test instead of silently retiring the path from the suite.

An operand is a C-order array over its labels (extents in `ext`); `a_off` elements of offset make A's
address 8 mod 16.  `out`: None (the C-order output the engine allocates), "T" (a transposed view: the
buffer is C-order over the reversed kept labels) or "pad" (a slice of a larger buffer, PAD_LO / PAD_HI extra
elements around every axis, or every other element of a 1-D buffer; the rest holds a sentinel).
"""

PAD_LO, PAD_HI = 1, 2
BASE_ADDR = 1 << 20  # a 16-B aligned stand-in address for the CPU test

FLAT, ROWS, ROWS_TAB, ROWS_TAB2 = 0, 1, 2, 3  # enum pgm_contract_kernel


def case(name, ext, la, lb, keep, reduce, combine, expect, a_off=0, out=None, gpu=True):
    return dict(name=name, ext=ext, la=list(la), lb=None if lb is None else list(lb), keep=list(keep), reduce=reduce,
                combine=combine, expect=expect, a_off=a_off, out=out, gpu=gpu)


CASES = [
    # ------------------------------------------------------------------ flat
    case("flat_g1_rollover", dict(a=8323, p=2, q=5, x=63), "apqx", "qp", "ax", "sum", "mul",
         dict(kernel=FLAT, g_log2=0, n_split=1, n_ro=2, ri_card=5)),  # 10 entries: rollover inside a group of 8
    case("flat_g2", dict(o=7, k=3), "ok", None, "o", "sum", "copy", dict(kernel=FLAT, g_log2=1, n_split=1)),
    case("flat_g64_ragged", dict(o=7, k=513), "ok", "k", "o", "sum", "mul",
         dict(kernel=FLAT, g_log2=6, n_split=1, n_ro=1)),  # lane 0 has 9 entries, the others 8
    case("flat_g64_two_keep", dict(o=7, m=3, k=513), "omk", "k", "om", "sum", "mul",
         dict(kernel=FLAT, g_log2=6, n_split=1)),
    case("flat_split_all_used", dict(p=37, o=5, q=50), "poq", None, "o", "sum", "copy",
         dict(kernel=FLAT, g_log2=5, n_split=37, red_chunk=1, empty_splits=0)),
    case("flat_split_empty", dict(p=2500, o=5, q=4), "poq", "pq", "o", "sum", "mul",
         dict(kernel=FLAT, n_split=1024, red_chunk=3, empty_splits=190)),
    case("flat_contig_reduction", dict(x=100, k=40), "xk", None, "x", "sum", "copy",
         dict(kernel=FLAT, g_log2=5)),  # NX >= 64, yet flat: the reduction is contiguous and the output small
    # ------------------------------------------------------------------ rows, no reduction
    case("rows_none_unrolled_1d", dict(x=1600001), "x", "x", "x", None, "mul",
         dict(kernel=ROWS, grid=(2048, 1, 1), unrolled=1)),
    case("rows_none_unrolled_outer", dict(o=1025, x=1027), "ox", "x", "ox", None, "mul",
         dict(kernel=ROWS, grid=(1, 1025, 1), unrolled=1)),
    case("rows_none_grid_y_wrap", dict(x=64, o=70000), "xo", None, "ox", None, "copy",
         dict(kernel=ROWS, grid=(1, 65535, 1), unrolled=0)),
    # ------------------------------------------------------------------ rows, LDS table
    case("rows_tab_tail_only", dict(k=5, x=64), "kx", None, "x", "sum", "copy",
         dict(kernel=ROWS_TAB, n_red=5), a_off=1),
    case("rows_tab_8_plus_tail", dict(k=13, o=3, x=100), "kox", "k", "ox", "sum", "mul",
         dict(kernel=ROWS_TAB, n_red=13)),
    case("rows_tab_full", dict(p=16, z=2, q=32, x=64, o=512), "pzqx", "o", "ozx", "sum", "mul",
         dict(kernel=ROWS_TAB, n_red=512, n_ro=16, n_split=1)),
    case("rows_over_tab", dict(p=19, z=2, q=27, x=64, o=512), "pzqx", "o", "ozx", "sum", "mul",
         dict(kernel=ROWS, n_red=513, n_split=1, ri_nb=1)),
    # the two shapes above as one dense operand (1 GiB each): plan only, too large for a quick GPU test
    case("rows_tab_full_dense", dict(p=16, o=128, q=32, x=2048), "poqx", None, "ox", "sum", "copy",
         dict(kernel=ROWS_TAB, n_red=512, n_ro=16, n_split=1), a_off=1, gpu=False),
    case("rows_over_tab_dense", dict(p=19, o=128, q=27, x=2048), "poqx", None, "ox", "sum", "copy",
         dict(kernel=ROWS, n_red=513, n_split=1, ri_nb=1), gpu=False),
    case("rows_tab2_odd_grid", dict(o=3, k=9, x=514), "okx", None, "ox", "sum", "copy",
         dict(kernel=ROWS_TAB2, n_red=9)),
    case("rows_tab2_misaligned", dict(o=3, k=9, x=514), "okx", None, "ox", "sum", "copy",
         dict(kernel=ROWS_TAB, n_red=9), a_off=1),
    # ------------------------------------------------------------------ rows, split
    case("rows_split_ragged", dict(k=4001, x=512), "kx", "k", "x", "sum", "mul",
         dict(kernel=ROWS, ri_nb=236, ri_chunk=17, n_split=236)),
    case("rows_split_v_decode", dict(p=3, k=700, x=512), "pkx", "p", "x", "sum", "mul",
         dict(kernel=ROWS, ri_nb=42, n_split=126)),
    case("rows_split_cross_ro", dict(p=7, k=650, x=512), "pkx", "p", "x", "sum", "mul",
         dict(kernel=ROWS, ri_nb=39, n_v=273, n_split=256, red_chunk=2)),
    case("rows_split_nb1", dict(p=40, o=2, k=30, x=300), "pokx", None, "ox", "sum", "copy",
         dict(kernel=ROWS, ri_nb=1, n_split=40)),
    # ------------------------------------------------------------------ strided out=
    case("flat_out_T", dict(o=7, m=3, k=513), "omk", "k", "om", "sum", "mul", dict(kernel=FLAT, g_log2=6), out="T"),
    case("flat_out_pad", dict(o=7, m=3, k=513), "omk", "k", "om", "sum", "mul", dict(kernel=FLAT, g_log2=6),
         out="pad"),
    case("flat_split_out_pad", dict(p=37, o=5, q=50), "poq", None, "o", "sum", "copy",
         dict(kernel=FLAT, n_split=37), out="pad"),
    case("rows_none_out_T", dict(o=1025, x=771), "ox", "x", "ox", None, "mul", dict(kernel=ROWS, unrolled=1), out="T"),
    case("rows_none_out_pad", dict(o=1025, x=771), "ox", "x", "ox", None, "mul", dict(kernel=ROWS, unrolled=1),
         out="pad"),
    case("rows_tab_out_T", dict(k=13, o=3, x=100), "kox", "k", "ox", "sum", "mul", dict(kernel=ROWS_TAB), out="T"),
    case("rows_tab_out_pad", dict(k=13, o=3, x=100), "kox", "k", "ox", "sum", "mul", dict(kernel=ROWS_TAB),
         out="pad"),
    case("rows_tab_copy_out_pad", dict(o=3, k=9, x=514), "okx", None, "ox", "sum", "copy",
         dict(kernel=ROWS_TAB), out="pad"),  # odd outer stride of C: not the two-rows-per-lane kernel
    case("rows_split_out_T", dict(p=40, o=2, k=30, x=300), "pokx", None, "ox", "sum", "copy",
         dict(kernel=ROWS, n_split=40), out="T"),
    case("rows_split_out_pad", dict(p=40, o=2, k=30, x=300), "pokx", None, "ox", "sum", "copy",
         dict(kernel=ROWS, n_split=40), out="pad"),
]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def c_strides(shape):
    st, acc = [], 1
    for c in reversed(shape):
        st.append(acc)
        acc *= c
    return st[::-1]


def operand_shapes(c):
    """(shape_a, shape_b): shape_b None without a second operand."""
    sa = [c["ext"][l] for l in c["la"]]
    sb = None if c["lb"] is None else [c["ext"][l] for l in c["lb"]]
    return sa, sb


def out_layout(c):
    """(buffer shape, view shape, view strides, view offset) of the output, in elements."""
    shape = [c["ext"][l] for l in c["keep"]]
    if c["out"] is None:
        return shape, shape, c_strides(shape), 0
    if c["out"] == "T":
        buf = shape[::-1]
        return buf, shape, c_strides(buf)[::-1], 0
    if len(shape) == 1:  # every other element of a 1-D buffer
        return [2 * shape[0] + PAD_LO + PAD_HI], shape, [2], PAD_LO
    buf = [s + PAD_LO + PAD_HI for s in shape]
    st = c_strides(buf)
    return buf, shape, st, sum(PAD_LO * s for s in st)


def info_args(c, a_ptr=None, c_ptr=None):
    """Positional and keyword arguments of engine.contract_info for this case (stand-in addresses with the
    case's alignment unless real ones are given)."""
    sa, sb = operand_shapes(c)
    _, _, ost, ooff = out_layout(c)
    return ((c["la"], sa, c_strides(sa), c["lb"], sb or (), c_strides(sb) if sb else (), c["keep"]),
            dict(reduce=c["reduce"], combine=c["combine"], out_stride=ost,
                 a_ptr=BASE_ADDR + 8 * c["a_off"] if a_ptr is None else a_ptr,
                 c_ptr=BASE_ADDR + 8 * ooff if c_ptr is None else c_ptr))


def features(info):
    """The path features of one plan (N.ContractInfo), the vocabulary of REQUIRED."""
    f = {("kernel", int(info.kernel))}
    if info.kernel == FLAT and info.n_red > 1:
        f.add(("flat_g1", info.g_log2 == 0))
        f.add(("flat_g", 1 << info.g_log2))
    if info.n_split > 1:
        f.add(("split", int(info.kernel)))
        if info.empty_splits:
            f.add(("empty_splits", int(info.kernel)))
        if info.kernel == ROWS:
            f.add(("rows_split_chunked", info.ri_nb > 1))
            if info.ri_nb > 1 and info.n_ro > 1:
                f.add("rows_split_v_decode")
            if info.red_chunk > 1 and info.ri_nb > 1 and info.n_ro > 1:
                f.add("rows_split_chunk_crosses_ro")
    if info.unrolled:
        f.add("rows_none_unrolled")
    if info.kernel != FLAT and info.grid[1] < info.n_out // info.nx:
        f.add("rows_grid_y_wrap")
    if info.kernel == ROWS_TAB:
        if info.n_red < 8:
            f.add("tab_tail_only")
        elif info.n_red % 8:
            f.add("tab_8_plus_tail")
        if info.n_red == 512:
            f.add("tab_full")
    if info.kernel == ROWS and info.n_red == 513 and info.n_split == 1:
        f.add("just_over_tab")
    return f


# every path the table exists for: the union of features() over the table must contain these
REQUIRED = [
    ("kernel", FLAT), ("kernel", ROWS), ("kernel", ROWS_TAB), ("kernel", ROWS_TAB2),
    ("flat_g1", True), ("flat_g", 2), ("flat_g", 64),
    ("split", FLAT), ("split", ROWS), ("empty_splits", FLAT), ("empty_splits", ROWS),
    ("rows_split_chunked", True), ("rows_split_chunked", False), "rows_split_v_decode", "rows_split_chunk_crosses_ro",
    "rows_none_unrolled", "rows_grid_y_wrap", "tab_tail_only", "tab_8_plus_tail", "tab_full", "just_over_tab",
]
