#!/usr/bin/env python3
"""Generate tests/golden/prim_plan.json: what the primitive planner decides for a seeded set of descriptors.

    PGM_LIB_PATH=/path/to/libpgmhip.so python tests/golden/make_golden_prim_plan.py

The file is a frozen record, made with the library built from the commit BEFORE the planner moved out of
pgmhip.hip into pgmprim_plan.cpp (PGM_LIB_PATH points at that build).  It is not regenerated from the code
under test: tests/test_prim_plan_cpu.py calls table() on the current library and requires the same table,
field by field.  Everything goes through the public, host-only entry points (no device is needed):

  binary   pgm_contract_info + pgm_contract_workspace for N_BINARY generated pgm_contract_desc: 0 .. 6 kept and
           reduced dims, extents that include 1, dense / permuted / padded / broadcast strides, every combine and
           reduce value, A and C addresses of 0 and 8 mod 16 (and NULL), plus hand-made edge descriptors
  nary     pgm_contract_n_info for N_NARY generated pgm_contractn_desc with 1 .. 8 operands
  batch    the pgm_batch_blocks total after each generated contraction, n-ary product, gather and n-ary
           contraction job added to a batch that is never finalized (stand-in addresses), in both batch modes:
           the 16-byte-pairs and lanes-per-output choices of the batch path show in the block counts
A rejected descriptor is recorded with its status and its error text.

The PGM_BATCH_* / PGM_NARY_LANES variables must be unset (the table is for the default caps).
"""
import ctypes
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "prim_plan.json")

SEED = 20261021
N_BINARY, N_NARY, N_BATCH = 2000, 400, 700
BASE = 0x7F0000000000  # stand-in device addresses: never dereferenced by the host-only entry points

SMALL = (1, 1, 2, 2, 2, 3, 3, 4, 5, 7, 8, 16)
WIDE_KEEP = (64, 100, 128, 255, 256, 257, 512, 1000, 4096, 100000)
LONG_RED = (64, 256, 512, 513, 1000, 4096, 8191, 8192, 3 * 8192, 16384, 65536, 1 << 20)

BINARY_FIELDS = ("kernel", "g_log2", "n_split", "red_chunk", "ri_nb", "ri_chunk", "grid0", "grid1", "grid2", "n_ro",
                 "n_v", "n_out", "n_red", "ri_card", "nx", "unrolled", "empty_splits", "workspace_bytes")
NARY_FIELDS = ("nk", "nr", "g_log2", "blocks", "n_out", "n_red", "kcard", "rcard")
BATCH_FIELDS = ("job", "status", "blocks_total")


def _strides(rng, extents, order, present, pad):
    """Strides of a dense array over the dims of `order` (outer -> inner) that are `present` (others 0:
    broadcast); pad: the innermost stride is 2, or one leading dimension is longer than its extent."""
    s = [0] * len(extents)
    run = 2 if pad == "inner" else 1
    for j, i in enumerate(reversed(order)):
        if not present[i]:
            continue
        s[i] = run
        run *= extents[i]
        if pad == "ld" and j == 0:
            run += rng.choice((1, 2, 3))
    return s


def _order(rng, nk, nr, how):
    keep, red = list(range(nk)), list(range(nk, nk + nr))
    if how == "keep_red":
        return keep + red
    if how == "red_keep":
        return red + keep
    o = keep + red
    rng.shuffle(o)
    return o


def _extents(rng, n, big):
    e = [rng.choice(SMALL) for _ in range(n)]
    if n and big is not None:
        e[-1] = big
    return e


def _addr(rng, null_ok=True):
    r = rng.random()
    if null_ok and r < 0.05:
        return None
    return BASE + rng.randrange(1 << 20) * 16 + (8 if r < 0.4 else 0)


def binary_desc(rng, N):
    """One generated pgm_contract_desc and its A, B, C stand-in addresses."""
    d = N.ContractDesc()
    d.combine, d.reduce = rng.randrange(5), rng.randrange(3)
    nk, nr = rng.randint(0, 6), rng.randint(0, 6)
    if d.reduce == N.RED_NONE and rng.random() < 0.9:
        nr = 0  # (reduced dims with RED_NONE are refused: a few stay)
    flavour = rng.choice(("plain", "plain", "wide", "long", "both"))
    ke = _extents(rng, nk, rng.choice(WIDE_KEEP) if flavour in ("wide", "both") else None)
    re_ = _extents(rng, nr, rng.choice(LONG_RED) if flavour in ("long", "both") else None)
    ext = ke + re_
    n = nk + nr
    hows = ("keep_red", "red_keep", "shuffle")
    pa = [rng.random() < 0.9 for _ in range(n)]
    pb = [rng.random() < 0.6 for _ in range(n)]
    sa = _strides(rng, ext, _order(rng, nk, nr, rng.choice(hows)), pa, rng.choice((None, None, None, "inner", "ld")))
    sb = _strides(rng, ext, _order(rng, nk, nr, rng.choice(hows)), pb, rng.choice((None, None, None, "inner", "ld")))
    oc = list(range(nk))
    if rng.random() < 0.4:
        rng.shuffle(oc)
    sc = _strides(rng, ke, oc, [True] * nk, rng.choice((None, None, None, "inner", "ld")))
    d.n_keep, d.n_red = nk, nr
    for i in range(nk):
        d.keep_card[i], d.keep_sa[i], d.keep_sb[i], d.keep_sc[i] = ke[i], sa[i], sb[i], sc[i]
    for i in range(nr):
        d.red_card[i], d.red_sa[i], d.red_sb[i] = re_[i], sa[nk + i], sb[nk + i]
    return d, _addr(rng), _addr(rng, False), _addr(rng)


def edge_binary_descs(N):
    """Hand-made descriptors at the planner's thresholds and refusals (appended to the generated ones)."""
    out = []

    def mk(keep, red, combine=N.COMBINE_COPY, reduce=N.RED_SUM, a=BASE, c=BASE):
        d = N.ContractDesc()
        d.combine, d.reduce, d.n_keep, d.n_red = combine, reduce, len(keep), len(red)
        for i, (card, s_a, s_b, s_c) in enumerate(keep):
            d.keep_card[i], d.keep_sa[i], d.keep_sb[i], d.keep_sc[i] = card, s_a, s_b, s_c
        for i, (card, s_a, s_b) in enumerate(red):
            d.red_card[i], d.red_sa[i], d.red_sb[i] = card, s_a, s_b
        out.append((d, a, BASE, c))
        return d

    for run in (8191, 8192, 8193, 12288, 16384, 1 << 20):  # the long-run split and its neighbours
        for outer in (1, 2, 255, 256):
            mk([(3, outer * run, 0, 1)], [(outer, 2 * run, 0), (run, 1, 0)] if outer > 1 else [(run, 1, 0)])
    for nx in (63, 64, 255, 256, 257, 512):  # row mode on and off, the two-row kernel's parity
        for nred in (1, 2, 511, 512, 513, 4096):
            for c_addr in (BASE, BASE + 8):
                mk([(4, nx * nred, 0, nx), (nx, 1, 0, 1)], [(nred, nx, 0)], c=c_addr)
            mk([(4, nx * nred, nx, nx), (nx, nred, 1, 1)], [(nred, 1, 0)], combine=N.COMBINE_MUL, reduce=N.RED_MAX)
    for n_out in (1, 1000, 131071, 131072, 524287, 524288, 1 << 22):  # lanes per output, split-K
        for nred in (2, 63, 64, 65, 1000):
            mk([(n_out, nred, 0, 1)], [(nred, 1, 0)])
            mk([(n_out, 1, 0, 1)], [(4, n_out * nred // 4 if nred % 4 == 0 else n_out * nred, 0), (nred, n_out, 0)])
    # KMAX dims that cannot merge, one more, and a dim that merges for A but not for C
    mk([(2, 1 << (2 * (11 - i)), 0, 1 << (2 * (11 - i))) for i in range(12)], [], reduce=N.RED_NONE)
    mk([(2, 1 << (2 * (12 - i)), 0, 1 << (2 * (12 - i))) for i in range(13)], [], reduce=N.RED_NONE)
    mk([(2, 1, 0, 1)], [(2, 1 << (2 * (12 - i)), 0) for i in range(13)])
    mk([(4, 8, 0, 16), (8, 1, 0, 1)], [], reduce=N.RED_NONE)
    # refusals
    mk([(0, 1, 0, 1)], [])
    mk([(4, 1, 0, 1)], [(-1, 1, 0)])
    mk([(4, 1, 0, 1)], [(0, 1, 0)])
    mk([(4, 1, 0, 1)], [(3, 4, 0)], reduce=N.RED_NONE)
    mk([(1 << 16, 1 << 15, 0, 1 << 15), (1 << 15, 1, 0, 1)], [])
    mk([(2, 1, 0, 1)], [(1 << 16, 1 << 15, 0), (1 << 15, 1, 0)])
    mk([(2, 1, 0, 1)], [], combine=5)
    mk([(2, 1, 0, 1)], [], reduce=3)
    mk([(2, 1, 0, 1)], []).n_keep = 33
    mk([(2, 1, 0, 1)], []).n_red = -1
    return out


def nary_desc(rng, N):
    d = N.ContractNDesc()
    d.n_ops = rng.randint(1, 8)
    d.reduce = rng.choice((N.RED_SUM, N.RED_MAX))
    nk, nr = rng.randint(0, 5), rng.randint(0, 4)
    flavour = rng.choice(("plain", "plain", "plain", "wide", "long"))
    ke = _extents(rng, nk, rng.choice((64, 256, 1000, 4096)) if flavour == "wide" else None)
    re_ = _extents(rng, nr, rng.choice((64, 256, 4096, 65536)) if flavour == "long" else None)
    ext, n = ke + re_, nk + nr
    d.n_keep, d.n_red = nk, nr
    for t in range(d.n_ops):
        present = [rng.random() < 0.7 for _ in range(n)]
        s = _strides(rng, ext, _order(rng, nk, nr, rng.choice(("keep_red", "keep_red", "red_keep", "shuffle"))), present,
                     rng.choice((None, None, None, None, "inner", "ld")))
        for i in range(nk):
            d.keep_s[t][i] = s[i]
        for i in range(nr):
            d.red_s[t][i] = s[nk + i]
    oc = list(range(nk))
    if rng.random() < 0.3:
        rng.shuffle(oc)
    sc = _strides(rng, ke, oc, [True] * nk, rng.choice((None, None, None, "ld")))
    for i in range(nk):
        d.keep_card[i], d.keep_sc[i] = ke[i], sc[i]
    for i in range(nr):
        d.red_card[i] = re_[i]
    r = rng.random()  # a few refusals and empty outputs
    if r < 0.02:
        d.reduce = N.RED_NONE
    elif r < 0.04:
        d.n_ops = rng.choice((0, 9))
    elif r < 0.06 and nk:
        d.keep_card[rng.randrange(nk)] = rng.choice((0, -1))
    elif r < 0.08 and nr:
        d.red_card[rng.randrange(nr)] = rng.choice((0, -2))
    elif r < 0.09:
        d.n_keep = 33
    return d


def edge_nary_descs(N):
    out = []
    for nd in (12, 13):  # KMAX unmergeable dims on each side, and one more
        for side in ("keep", "red"):
            d = N.ContractNDesc()
            d.n_ops, d.reduce = 2, N.RED_SUM
            for i in range(nd):
                s = 1 << (2 * (nd - 1 - i))
                if side == "keep":
                    d.keep_card[i], d.keep_sc[i], d.keep_s[0][i] = 2, s, s
                else:
                    d.red_card[i], d.red_s[0][i], d.red_s[1][i] = 2, s, 2 * s
            d.n_keep, d.n_red = (nd, 0) if side == "keep" else (0, nd)
            out.append(d)
    for n_out in (1, 255, 256, 16383, 16384, 1 << 20):  # lanes per output against the lanes cap and n_red
        for n_red in (1, 2, 63, 64, 1000):
            d = N.ContractNDesc()
            d.n_ops, d.reduce, d.n_keep, d.n_red = 1, N.RED_SUM, 1, 1
            d.keep_card[0], d.keep_sc[0], d.keep_s[0][0] = n_out, 1, n_red
            d.red_card[0], d.red_s[0][0] = n_red, 1
            out.append(d)
    d = N.ContractNDesc()  # a negative extent behind an empty kept dim: the empty output wins
    d.n_ops, d.reduce, d.n_keep = 1, N.RED_SUM, 2
    d.keep_card[0], d.keep_card[1] = -1, 0
    out.append(d)
    d = N.ContractNDesc()  # over 2^31 outputs / reduced entries
    d.n_ops, d.reduce, d.n_keep = 1, N.RED_SUM, 2
    d.keep_card[0], d.keep_card[1], d.keep_sc[0], d.keep_sc[1] = 1 << 16, 1 << 15, 1 << 16, 1
    out.append(d)
    d = N.ContractNDesc()
    d.n_ops, d.reduce, d.n_red = 1, N.RED_MAX, 2
    d.red_card[0], d.red_card[1], d.red_s[0][0], d.red_s[0][1] = 1 << 16, 1 << 15, 1 << 16, 1
    out.append(d)
    return out


def productn_desc(rng, N):
    """A generated pgm_productn_desc and its operand / output stand-in addresses."""
    d = N.ProductNDesc()
    d.n_ops = rng.randint(1, 8)
    nk = rng.randint(0, 5)
    ke = _extents(rng, nk, rng.choice((2, 6, 64, 100, 256, 1000)) if rng.random() < 0.6 else None)
    t = 0
    while t < d.n_ops:  # kinds: MUL, or a RATIO followed by its DEN
        if t + 1 < d.n_ops and rng.random() < 0.2:
            d.op_kind[t], d.op_kind[t + 1] = N.PRODN_RATIO, N.PRODN_DEN
            t += 2
        else:
            d.op_kind[t] = N.PRODN_MUL
            t += 1
    d.n_keep = nk
    for t in range(d.n_ops):
        present = [rng.random() < 0.75 for _ in range(nk)]
        order = list(range(nk))
        if rng.random() < 0.25:
            rng.shuffle(order)
        s = _strides(rng, ke, order, present, rng.choice((None, None, None, None, "inner", "ld")))
        for i in range(nk):
            d.keep_s[t][i] = s[i]
    oc = list(range(nk))
    if rng.random() < 0.15:
        rng.shuffle(oc)
    sc = _strides(rng, ke, oc, [True] * nk, rng.choice((None, None, None, None, "inner", "ld")))
    for i in range(nk):
        d.keep_card[i], d.keep_sc[i] = ke[i], sc[i]
    r = rng.random()
    if r < 0.02 and nk:
        d.keep_card[rng.randrange(nk)] = 0
    elif r < 0.04:
        d.op_kind[0] = N.PRODN_DEN
    elif r < 0.05:
        d.n_ops = 9
    ops = (ctypes.c_void_p * 8)(*[BASE + rng.randrange(1 << 20) * 16 + (8 if rng.random() < 0.1 else 0) for _ in range(8)])
    if rng.random() < 0.02:
        ops[0] = None
    return d, ops, BASE + rng.randrange(1 << 20) * 16 + (8 if rng.random() < 0.1 else 0)


def gather_desc(rng, N):
    d = N.GatherDesc()
    nk = rng.randint(0, 6)
    ke = _extents(rng, nk, rng.choice((64, 1000, 100000)) if rng.random() < 0.5 else None)
    d.n_keep, d.n_ev = nk, rng.randint(0, 4)
    d.batch_dim = rng.randint(-1, nk - 1) if nk else -1
    d.ld, d.row0 = 1 << 20, rng.randrange(1000)
    s = _strides(rng, ke, list(range(nk)), [True] * nk, None)
    for i in range(nk):
        d.keep_card[i], d.keep_sa[i], d.keep_sc[i] = ke[i], 3 * s[i], s[i]
    for j in range(d.n_ev):
        d.ev_col[j], d.ev_stride[j], d.ev_card[j] = j, 7 * (j + 1), rng.randint(2, 5)
    r = rng.random()
    if r < 0.03:
        d.n_keep = 13
    elif r < 0.06:
        d.batch_dim = nk
    elif r < 0.09 and nk:
        d.keep_card[0] = 0
    return d


def _digest(h, struct):
    h.update(bytes(struct))


def _err(N):
    return N.last_error()


def table(N=None):
    """The whole table as the JSON-ready dict, from the library pgmpy_amd._native loads."""
    if N is None:
        sys.path.insert(0, ROOT)
        from pgmpy_amd import _native as N
    for v in ("PGM_BATCH_LANES_CAP", "PGM_BATCH_MAX_BLOCKS", "PGM_BATCH_MAX_BLOCKS_PRODUCT", "PGM_NARY_LANES"):
        assert not os.environ.get(v), f"{v} is set: the table is for the default caps"
    lib = N.load_library()
    P = ctypes.c_void_p

    # ---- binary contractions
    rng = random.Random(SEED)
    descs = [binary_desc(rng, N) for _ in range(N_BINARY)] + edge_binary_descs(N)
    h = hashlib.sha256()
    rows = []
    for d, a, _b, c in descs:
        _digest(h, d)
        h.update(repr((a, c)).encode())
        info, ws = N.ContractInfo(), ctypes.c_size_t(0)
        rc = lib.pgm_contract_info(ctypes.byref(d), P(a), P(c), ctypes.byref(info))
        if rc != N.PGM_OK:
            rows.append([rc, _err(N)])
            continue
        assert lib.pgm_contract_workspace(ctypes.byref(d), ctypes.byref(ws)) == N.PGM_OK
        rows.append([info.kernel, info.g_log2, info.n_split, info.red_chunk, info.ri_nb, info.ri_chunk, *info.grid,
                     info.n_ro, info.n_v, info.n_out, info.n_red, info.ri_card, info.nx, info.unrolled,
                     info.empty_splits, ws.value])
    binary = {"fields": list(BINARY_FIELDS), "inputs_sha256": h.hexdigest(), "rows": rows}

    # ---- n-ary contractions
    rng = random.Random(SEED + 1)
    ndescs = [nary_desc(rng, N) for _ in range(N_NARY)] + edge_nary_descs(N)
    h = hashlib.sha256()
    rows = []
    for d in ndescs:
        _digest(h, d)
        info = N.ContractNInfo()
        rc = lib.pgm_contract_n_info(ctypes.byref(d), None, ctypes.byref(info))
        if rc != N.PGM_OK:
            rows.append([rc, _err(N)])
            continue
        rows.append([info.nk, info.nr, info.g_log2, info.blocks, info.n_out, info.n_red,
                     list(info.kcard[:max(info.nk, 0)]), list(info.rcard[:max(info.nr, 0)])])
    nary = {"fields": list(NARY_FIELDS), "inputs_sha256": h.hexdigest(), "rows": rows}

    # ---- batch jobs: the running block total of a batch that is never finalized
    batch = {"fields": list(BATCH_FIELDS)}
    for mode_name, mode in (("grid", N.BATCH_GRID), ("one_workgroup", N.BATCH_ONE_WORKGROUP)):
        rng = random.Random(SEED + 2)
        h = hashlib.sha256()
        handle = P()
        assert lib.pgm_batch_create(ctypes.byref(handle)) == N.PGM_OK
        assert lib.pgm_batch_set_mode(handle, mode) == N.PGM_OK
        rows = []
        edge = edge_binary_descs(N)
        for j in range(N_BATCH):
            kind = rng.choice("cccccppppgn")
            if kind == "c":
                d, a, b, c = binary_desc(rng, N) if rng.random() < 0.85 else edge[rng.randrange(len(edge))]
                a = a or BASE
                c = c or BASE + 16
                _digest(h, d)
                h.update(repr((a, b, c)).encode())
                rc = lib.pgm_batch_add_contract(handle, ctypes.byref(d), P(a), P(b), P(c))
            elif kind == "p":
                d, ops, c = productn_desc(rng, N)
                _digest(h, d)
                h.update(repr((list(ops), c)).encode())
                rc = lib.pgm_batch_add_product_n(handle, ctypes.byref(d), ops, P(c))
            elif kind == "g":
                d = gather_desc(rng, N)
                _digest(h, d)
                rc = lib.pgm_batch_add_gather(handle, ctypes.byref(d), P(BASE), P(BASE + 4096), P(BASE + 8192), None)
            else:
                d = nary_desc(rng, N)
                _digest(h, d)
                ops = (ctypes.c_void_p * 8)(*[BASE + 64 * (t + 1) for t in range(8)])
                rc = lib.pgm_batch_add_contract_n(handle, ctypes.byref(d), ops, P(BASE))
            blocks = ctypes.c_int64(-1)
            assert lib.pgm_batch_blocks(handle, ctypes.byref(blocks)) == N.PGM_OK
            rows.append([kind, rc, blocks.value] if rc == N.PGM_OK else [kind, rc, blocks.value, _err(N)])
            if mode == N.BATCH_ONE_WORKGROUP and j % 50 == 49:
                assert lib.pgm_batch_add_level(handle) == N.PGM_OK
        assert lib.pgm_batch_destroy(handle) == N.PGM_OK
        batch[mode_name] = {"inputs_sha256": h.hexdigest(), "rows": rows}

    return {"what": "the primitive planner's decisions for the seeded descriptors of tests/golden/make_golden_prim_plan.py, "
                    "recorded with the library built from the commit before the planner moved out of pgmhip.hip "
                    "into pgmprim_plan.cpp; a rejected descriptor is [status, error text]",
            "seed": SEED, "binary": binary, "nary": nary, "batch": batch}


def summary(t):
    """Counts that show what the generated set reaches (printed by the generator, asserted by the test)."""
    ok = [r for r in t["binary"]["rows"] if len(r) == len(BINARY_FIELDS)]
    f = {n: i for i, n in enumerate(BINARY_FIELDS)}
    s = {"binary": len(t["binary"]["rows"]), "binary_rejected": len(t["binary"]["rows"]) - len(ok)}
    for k in range(4):
        s[f"kernel_{k}"] = sum(r[f["kernel"]] == k for r in ok)
    s["split"] = sum(r[f["n_split"]] > 1 for r in ok)
    s["ri_nb"] = sum(r[f["ri_nb"]] > 1 for r in ok)
    s["g_log2"] = sorted({r[f["g_log2"]] for r in ok})
    s["nary"] = len(t["nary"]["rows"])
    s["nary_rejected"] = sum(len(r) == 2 for r in t["nary"]["rows"])
    s["nary_g_log2"] = sorted({r[2] for r in t["nary"]["rows"] if len(r) != 2})
    for m in ("grid", "one_workgroup"):
        rows = t["batch"][m]["rows"]
        s[f"batch_{m}"] = (len(rows), sum(r[1] != 0 for r in rows), rows[-1][2])
    return s


if __name__ == "__main__":
    t = table()
    with open(OUT, "w") as fh:
        json.dump(t, fh, separators=(",", ":"))
        fh.write("\n")
    print(json.dumps(summary(t)))
    print(OUT, os.path.getsize(OUT), "bytes")
