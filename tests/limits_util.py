"""Inputs and exact checks for the raw-limb op table of tests/device/limit_ops.h (helper module, not a conftest).

The table is run by two builds of the same source: the host driver tests/host/fp_limits_host_test.hip (tests/test_limits_host.py) and
gs_prim_run_raw of tests/device/prim_test.hip (tests/test_gpu_primitives.py).  Everything here is Python integers and exact identities.

Contract as coded (csrc/fp29.h, top of the file): an Fe<M, B> has value < B p and limbs 0..7 <= kNearlyNormalMax - 1 = 2^29 + 7 (SAT
below, checked against the constant the build holds); an Lz<., ., W> only arises from the lazy ops on such inputs.  Every operand generated here is asserted against that contract before it is sent.
Operand classes: saturated / zero / mixed low limbs under the largest top limb that keeps the value below B p; the values k p + delta for
every k < B in normal form; and, for subtrahends, zero low limbs against saturated ones (both ways)."""
import itertools
import os
import random
import re
import struct
import subprocess

import numpy as np

from oracle import ref_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "device", "limit_ops.h")
NL, LB = 9, 29
MASK = (1 << LB) - 1
SAT = (1 << LB) + 7                     # the largest low limb an Fe may hold: kNearlyNormalMax - 1
MONT_R = 1 << (NL * LB)
IN_SLOTS, OUT_SLOTS = 8, 4
MODS = {0: O.Q, 1: O.R, 2: O.Q}


def in_words(kind):
    return IN_SLOTS * NL if kind < 3 else (8 * NL if kind == 3 else 16 * NL)


def out_words(kind):
    return OUT_SLOTS * NL + IN_SLOTS if kind < 3 else (4 * NL if kind == 3 else 8 * NL)


def value(limbs):
    return sum(int(v) << (LB * i) for i, v in enumerate(limbs))


def normal_limbs(v):
    assert 0 <= v < 1 << (LB * (NL - 1) + 32)
    return [(v >> (LB * i)) & MASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]


def assert_fe(limbs, bound, p, low_max=SAT, at_bound=False):
    """the input contract of an Fe<M, bound> (low_max = 2^29 - 1 for an op that wants fully normalised limbs; at_bound: the one value
    the header admits AT B p, which neg / neg_lazy of zero leaves)"""
    assert len(limbs) == NL and all(0 <= v <= low_max for v in limbs[:NL - 1]) and 0 <= limbs[NL - 1] < 1 << 32, limbs
    assert value(limbs) < bound * p or (at_bound and value(limbs) == bound * p), (limbs, bound)


# ---- the op table, read from the header --------------------------------------------------------------------------------------------
class Op:
    def __init__(self, kind_set, op_id, name):
        self.kinds, self.id, self.name = kind_set, op_id, name
        self.base, _, digits = name.partition("__")
        self.bounds = [int(d) for d in digits.split("_")] if digits else []

    def __repr__(self):
        return self.name


def parse_ops():
    """LIMIT_OP(id, name) lines -> [Op]; kinds by table: fq2_* are the Fq2 table (kind 2), madd_u2s2* q only, the rest q and r"""
    text = open(HEADER).read()
    ops = []
    for m in re.finditer(r"^\s*LIMIT_OP\((\d+),\s*(\w+)\)", text, re.M):
        name = m.group(2)
        kinds = (2,) if name.startswith("fq2_") else (0,) if name.startswith("madd_u2s2") else (0, 1)
        ops.append(Op(kinds, int(m.group(1)), name))
    return ops


def family_ops(tables):
    """neg_lazy<B> (100 + B) and sub_lazy<2, B> (200 + B) at every B the tables admit -- every k with tbias_k(k) != k included"""
    ops = []
    for b in range(1, tables.max_k):
        ops.append(Op((tables.kind,), 100 + b, "neg_lazy__%d" % b))
        if 2 + tables.tbias_k[b + 1] <= tables.max_k:
            ops.append(Op((tables.kind,), 200 + b, "sub_lazy__2_%d" % b))
    return ops


# ---- running records ---------------------------------------------------------------------------------------------------------------
def host_run(exe, batches):
    """batches: [(kind, op id, uint32 array n x in_words)] -> [uint32 array n x out_words]"""
    blob = b"".join(struct.pack("<3I", k, o, len(a)) + np.ascontiguousarray(a, dtype="<u4").tobytes() for k, o, a in batches)
    out = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout
    res, at = [], 0
    for k, _, a in batches:
        n = len(a) * out_words(k)
        res.append(np.frombuffer(out, dtype="<u4", count=n, offset=at).reshape(len(a), out_words(k)))
        at += 4 * n
    assert at == len(out)
    return res


def pack_field(cases):
    """cases: [[limbs per slot]] -> n x 72"""
    a = np.zeros((len(cases), IN_SLOTS * NL), dtype=np.uint32)
    for i, c in enumerate(cases):
        flat = [v for s in c for v in s]
        a[i, :len(flat)] = flat
    return a


class Tables:
    """bias / tbias / wbias as the BUILD holds them (op 0 of the table), checked against k p"""

    def __init__(self, kind, run):
        self.kind, self.p = kind, MODS[kind]
        a = np.zeros((64, IN_SLOTS * NL), dtype=np.uint32)
        a[:, 0] = np.arange(64)
        out = run(kind, 0, a)
        self.max_k, self.top_limb, self.nearly_normal_max = int(out[1][3 * NL + 2]), int(out[1][3 * NL + 1]), int(out[1][3 * NL + 3])
        self.bias = {k: [int(v) for v in out[k][0:NL]] for k in range(1, self.max_k + 1)}
        self.tbias = {k: [int(v) for v in out[k][NL:2 * NL]] for k in range(1, self.max_k + 1)}
        self.wbias = {k: [int(v) for v in out[k][2 * NL:3 * NL]] for k in range(1, self.max_k + 1)}
        self.tbias_k = {k: int(out[k][3 * NL]) for k in range(1, self.max_k + 1)}

    def check(self):
        p = self.p
        assert self.max_k == 40 and self.top_limb == p >> (LB * (NL - 1)) and self.nearly_normal_max == SAT + 1
        for k in range(1, self.max_k + 1):
            assert value(self.bias[k]) == k * p and value(self.wbias[k]) == k * p
            assert k <= self.tbias_k[k] <= self.max_k and value(self.tbias[k]) == self.tbias_k[k] * p
            assert all((1 << LB) + 15 <= v < 1 << 30 for v in self.tbias[k][:NL - 1])       # K p - a: no underflow, limbs of weight 2
            assert all(v >= SAT for v in self.bias[k][:NL - 1]) and all(v >= 3 * SAT for v in self.wbias[k][:NL - 1])


# ---- operands ----------------------------------------------------------------------------------------------------------------------
LOW_CHOICES = [SAT, SAT - 1, 1 << LB, MASK, 1, 0, None]      # None: uniform


def _top_max(low, bound, p):
    return (bound * p - 1 - value(low + [0])) >> (LB * (NL - 1))


def limb_operands(rng, bound, p, low_max=SAT, mixes=6):
    """[(limbs, tags)]: low-limb classes x top-limb classes {largest with value < B p, that - 1, 0, uniform}"""
    choices = [c for c in LOW_CHOICES if c is None or c <= low_max] + ([low_max] if low_max != SAT else [])
    lows = [([low_max] * 8, "sat"), ([0] * 8, "zero")]
    for _ in range(mixes):
        lows.append(([rng.randrange(low_max + 1) if c is None else c for c in (rng.choice(choices) for _ in range(8))], "mix"))
    res = []
    for low, tag in lows:
        tmax = _top_max(low, bound, p)
        assert tmax >= 1
        for top, ttag in ((tmax, "max"), (tmax - 1, "max-1"), (0, "0"), (rng.randrange(tmax + 1), "uni")):
            res.append((low + [top], {tag + "_" + ttag}))
    return res


def value_operands(rng, bound, p):
    """k p + delta for every k < B (and B p - 1), delta in {-1, 0, +1, small random}, normal form"""
    res = []
    for k in range(bound + 1):
        for d in (-1, 0, 1, rng.randrange(2, 1 << 20)):
            v = k * p + d
            if 0 <= v < bound * p:
                res.append((normal_limbs(v), {"kp_pm1" if abs(d) == 1 else "kp" if d == 0 else "kp_small"}))
    return res


def operands(rng, bound, p, low_max=SAT):
    return limb_operands(rng, bound, p, low_max) + value_operands(rng, bound, p)


def field_cases(rng, op, p, low_max=SAT):
    """[(slots, tags)] for one op: every candidate of every slot once (the other slots drawn at random), all slots saturated at their
    largest top limb, all zero, and -- for two and three operand ops -- the underflow pairs and pairs that are equal mod p"""
    cands = [operands(rng, b, p, low_max) for b in op.bounds]
    cases = []
    for j, cj in enumerate(cands):
        for limbs, tags in cj:
            slots = [limbs if i == j else rng.choice(ci)[0] for i, ci in enumerate(cands)]
            cases.append((slots, tags if len(cands) == 1 else tags | {"slot%d" % j}))
    cases.append(([c[0][0] for c in cands], {"all_sat_max"}))                      # limb_operands' first entry: saturated, top max
    cases.append(([[0] * NL for _ in cands], {"all_zero"}))
    if len(cands) >= 2:
        sat = [[low_max] * 8 + [_top_max([low_max] * 8, b, p)] for b in op.bounds]
        zero_low = [[0] * 8 + [_top_max([0] * 8, b, p)] for b in op.bounds]
        for j in range(len(cands)):                                                # one slot with zero low limbs against saturated others
            cases.append(([zero_low[i] if i == j else sat[i] for i in range(len(cands))], {"underflow_pair"}))
            cases.append(([sat[i] if i == j else zero_low[i] for i in range(len(cands))], {"underflow_pair"}))
            cases.append(([zero_low[i] if i == j else [low_max] * 8 + [0] for i in range(len(cands))], {"underflow_pair"}))
        for _ in range(24):                                                        # slot 1 == slot 0 (mod p), every representation
            a = rng.choice(cands[0])[0]
            k = rng.randrange(op.bounds[1])
            slots = [a, normal_limbs(value(a) % p + k * p)] + [rng.choice(c)[0] for c in cands[2:]]
            cases.append((slots, {"equal_mod_p"}))
    if op.base in AT_BOUND:                                                        # fp29.h: "one value sits AT its bound", K p - 0
        for j, b in enumerate(op.bounds):
            cases.append(([normal_limbs(b * p) if i == j else rng.choice(ci)[0] for i, ci in enumerate(cands)], {"at_bound"}))
        cases.append(([normal_limbs(b * p) for b in op.bounds], {"at_bound"}))
    for slots, tags in cases:
        for limbs, b in zip(slots, op.bounds):
            assert_fe(limbs, b, p, low_max, at_bound="at_bound" in tags)
    return cases


# the consumers the header names for a value of exactly B p (neg / neg_lazy of zero): each takes one operand, and all of them, there
AT_BOUND = ("reduce2", "reduce2_normal", "canon", "is_zero", "mul", "sqr", "mul_add")


# ---- limb-exact models of the carry ops --------------------------------------------------------------------------------------------
def _u32(t):
    assert 0 <= t < 1 << 32, "a limb formula leaves [0, 2^32): %d" % t
    return t


def _carry_save(t):
    r = [v & MASK for v in t[:NL - 1]] + [t[NL - 1]]
    for i in range(1, NL):
        r[i] = _u32(r[i] + (t[i - 1] >> LB))
    return r


def _ripple(t_of):
    r, c = [], 0
    for i in range(NL):
        t = _u32(t_of(i) + c)
        if i < NL - 1:
            r.append(t & MASK)
            c = t >> LB
        else:
            r.append(t)
    return r


def carry_model(op, tb, s):
    """-> (expected limbs, expected integer value, value bound, limb rule) ; limb rule: 'cs' carry-save, 'normal', or lazy weight W"""
    p, b, v = tb.p, op.bounds, [value(x) for x in s]
    base = op.base
    lazy = {"add_lazy": 2, "dbl_lazy": 2, "neg_lazy": 2, "sub_lazy": 3}
    norm = base.startswith("normalize_")
    if norm:
        base = base[len("normalize_"):]
    if base in ("add", "add_lazy"):
        t, val, bound = [_u32(x + y) for x, y in zip(s[0], s[1])], v[0] + v[1], b[0] + b[1]
    elif base in ("dbl", "dbl_lazy"):
        t, val, bound = [_u32(2 * x) for x in s[0]], 2 * v[0], 2 * b[0]
    elif base in ("sub", "sub_ripple"):
        bias = tb.bias[b[1] + 1]
        t, val, bound = [x + _u32(bi - y) for x, y, bi in zip(s[0], s[1], bias)], v[0] - v[1] + (b[1] + 1) * p, b[0] + b[1] + 1
        if base == "sub_ripple":
            return _ripple(lambda i: t[i]), val, bound, "normal"
        t = [_u32(x) for x in t]
    elif base == "neg":
        t, val, bound = [_u32(bi - x) for x, bi in zip(s[0], tb.bias[b[0] + 1])], (b[0] + 1) * p - v[0], b[0] + 1
    elif base == "neg_lazy":
        kk = tb.tbias_k[b[0] + 1]
        t, val, bound = [_u32(bi - x) for x, bi in zip(s[0], tb.tbias[b[0] + 1])], kk * p - v[0], kk
    elif base == "sub_lazy":
        kk = tb.tbias_k[b[1] + 1]
        t = [_u32(x + _u32(bi - y)) for x, y, bi in zip(s[0], s[1], tb.tbias[b[1] + 1])]
        val, bound = v[0] - v[1] + kk * p, b[0] + kk
    elif base == "sub_b_2c":
        k = b[1] + 2 * b[2] + 1
        t = [_u32(x + _u32(bi - (2 * z + y))) for x, y, z, bi in zip(s[0], s[1], s[2], tb.wbias[k])]
        val, bound = v[0] - v[1] - 2 * v[2] + k * p, b[0] + k
    else:
        raise KeyError(op.name)
    if base in lazy and not norm:
        return t, val, bound, lazy[base]
    return _carry_save(t), val, bound, "cs"


CARRY = ("add", "dbl", "sub", "neg", "sub_ripple", "sub_b_2c", "add_lazy", "dbl_lazy", "neg_lazy", "sub_lazy")


def is_carry(op):
    return op.base in CARRY or op.base.startswith("normalize_")


# ---- numerators of the Montgomery ops: out_j R == N_j (mod p) ----------------------------------------------------------------------
MONT = {
    "mul": lambda a, b: [a * b],
    "sqr": lambda a: [a * a],
    "mul_add": lambda a, b, c, d: [a * b + c * d],
    "dot4": lambda a, b, c, d, e, f, g, h: [a * b + c * d + e * f + g * h],
    "mul_sub": lambda a, b, c, d: [a * b - c * d],
    "sqr2": lambda a, b: [a * a, b * b],
    "mul_lazy_w3w2": lambda a, b, c: [(a - b) * -c],
    "mul_lazy_w2w3": lambda a, b, c: [(a - b) * -c],
    "mul_lazy_w3fe": lambda a, b, c: [(a - b) * c],
    "mul_lazy_w2w2": lambda a, b, c: [(a + b) * 2 * c],
    "dots2": lambda a, b, c, d, e, f: [a * b + c * d, e * f],
    "dots3": lambda a, b, c, d, e, f, g, h: [a * b + c * d, e * f, g * h],
    "chains_fq2_sqr": lambda a, b: [(a + b) * (a - b), 2 * a * b],
    "chains_fq2_mul_sub": lambda a0, a1, b0, b1, c0, c1, d0, d1: [a0 * b0 - a1 * b1 - c0 * d0 + c1 * d1, a0 * b1 + a1 * b0 - c0 * d1 - c1 * d0],
    "dots_uniform_4_1": lambda a, b, c, d: [(a + b) * (a - b), 2 * a * b, (c + d) * (c - d), 2 * c * d],
    "dots_uniform_4_2": lambda a0, a1, b0, b1, c0, c1, d0, d1: [a0 * b0 - a1 * b1, a0 * b1 + a1 * b0, c0 * d0 - c1 * d1, c0 * d1 + c1 * d0],
    "madd_ppp_q": lambda P, PP, x: [P * PP, x * PP],
    "madd_y3": lambda R, Q, X3, y, PPP, zz, PP, zzz: [R * (Q - X3) - y * PPP, zz * PP, zzz * PPP],
    "madd_u2s2": lambda bx, zz, by, zzz: [bx * zz, by * zzz],
    "madd_u2s2_negate": lambda bx, zz, by, zzz: [bx * zz, -by * zzz],
}


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _csub(a, b):
    return (a[0] - b[0], a[1] - b[1])


FQ2 = {                                  # numerators as complex pairs, flattened (c0, c1) per output element
    "fq2_mul": lambda a, b: [_cmul(a, b)],
    "fq2_sqr": lambda a: [_cmul(a, a)],
    "fq2_mul_sub": lambda a, b, c, d: [_csub(_cmul(a, b), _cmul(c, d))],
    "fq2_mul2": lambda a, b, c, d: [_cmul(a, b), _cmul(c, d)],
    "fq2_sqr2": lambda a, b: [_cmul(a, a), _cmul(b, b)],
}


def assert_mont_out(limbs, p, what):
    assert all(0 <= v <= MASK for v in limbs[:NL - 1]) and value(limbs) < 2 * p, "%s: not a normal value below 2p: %s" % (what, limbs)


# ---- checking one op's records -----------------------------------------------------------------------------------------------------
def check_field_op(op, kind, tb, cases, out):
    """cases: [(slots, tags)], out: n x 44 array from either build.  Exact, no tolerance."""
    p = tb.p
    nb = len(op.bounds)
    sub_bounds = op.bounds if kind != 2 else [b for b in op.bounds for _ in (0, 1)]
    for (slots, tags), rec in zip(cases, out):
        rec = [int(v) for v in rec]
        what = "%s %s %s" % (op.name, sorted(tags), slots)
        o = [rec[NL * j:NL * (j + 1)] for j in range(OUT_SLOTS)]
        assert rec[OUT_SLOTS * NL:OUT_SLOTS * NL + len(sub_bounds)] == sub_bounds, "%s: the build read other bounds %s" % (op.name, rec[OUT_SLOTS * NL:])
        vals = [value(s) for s in slots]
        if kind == 2:
            pairs = [(vals[2 * i], vals[2 * i + 1]) for i in range(nb)]
            if op.base == "fq2_inv":
                prod = _cmul((value(o[0]), value(o[1])), pairs[0])
                zero = pairs[0][0] % p == 0 and pairs[0][1] % p == 0
                assert (prod[0] - (0 if zero else MONT_R * MONT_R)) % p == 0 and prod[1] % p == 0, what
                nums = []
            else:
                nums = [c for e in FQ2[op.base](*pairs) for c in e]
            for j in range(2 * (1 if op.base == "fq2_inv" else len(nums) // 2)):
                assert_mont_out(o[j], p, what)
            for j, n in enumerate(nums):
                assert (value(o[j]) * MONT_R - n) % p == 0, what
        elif is_carry(op):
            want, val, bound, rule = carry_model(op, tb, slots)
            if rule == "cs":                                      # what carry_save leaves
                assert o[0][0] <= MASK and all(v < (1 << LB) + 8 for v in o[0][1:NL - 1]), what + ": carry-save limbs"
            elif rule == "normal":
                assert all(v <= MASK for v in o[0][:NL - 1]), what + ": limbs not normal"
            else:
                assert all(v <= rule * (1 << LB) + 15 for v in o[0]), what + ": a limb above its weight %d" % rule
            assert o[0] == want, "%s: limbs %s, limb-wise formula gives %s" % (what, o[0], want)
            assert value(o[0]) == val and 0 <= val <= bound * p, what
            assert val < bound * p or (op.base.endswith(("neg", "neg_lazy")) and vals[0] == 0), what    # K p - 0: the one value AT its bound
        elif op.base in ("reduce2", "reduce2_normal"):
            assert_mont_out(o[0], p, what)
            assert (value(o[0]) - vals[0]) % p == 0, what
        elif op.base == "canon":
            assert o[0] == normal_limbs(vals[0] % p), what
        elif op.base == "is_zero":
            z = vals[0] % p == 0
            assert o[0][0] == int(z), what
            assert o[1][0] == 1 or not z, what + ": maybe_zero says no to a true zero"
        elif op.base == "equal":
            assert o[0][0] == int((vals[0] - vals[1]) % p == 0), what
        elif op.base == "inv":
            assert_mont_out(o[0], p, what)
            assert (value(o[0]) * vals[0] - (0 if vals[0] % p == 0 else MONT_R * MONT_R)) % p == 0, what
        else:
            nums = MONT[op.base](*vals)
            for j, n in enumerate(nums):
                assert_mont_out(o[j], p, what)
                assert (value(o[j]) * MONT_R - n) % p == 0, what


def assert_coverage(op, cases):
    """no case is dropped after generation; every op sees an all-saturated operand at its largest top limb and a k p +- 1"""
    tags = set().union(*(t for _, t in cases))
    assert "sat_max" in tags and "all_sat_max" in tags and "kp_pm1" in tags, (op.name, sorted(tags))
    assert ("at_bound" in tags) == (op.base in AT_BOUND), op.name


def low_max_of(op):
    return MASK if op.base == "reduce2_normal" else SAT          # reduce2_normal takes sub_ripple's result: limbs 0..7 below 2^29


def field_plan(kind, tb, seed):
    """[(op, cases)] for one field kind; an Fq2 op's slots are (c0, c1) per element, each with the element's bound"""
    rng = random.Random(seed)
    ops = [o for o in parse_ops() if kind in o.kinds and o.name != "tables"]
    if kind != 2:
        ops += family_ops(tb)
    plan = []
    for op in ops:
        gen = op if kind != 2 else Op(op.kinds, op.id, op.base + "__" + "_".join(str(b) for b in op.bounds for _ in (0, 1)))
        cases = field_cases(rng, gen, tb.p, low_max_of(op))
        assert_coverage(op, cases)
        plan.append((op, cases))
    return plan


# ---- points ------------------------------------------------------------------------------------------------------------------------
POINT_OPS = {0: "madd", 1: "madd_negate", 2: "add", 3: "add_mem", 4: "dbl", 5: "tight_madd", 6: "tight_madd_negate"}
XYZZ_BOUNDS = (9, 5, 2, 2)
TIGHT_BOUNDS = (9, 2, 2, 2)


class Curve:
    def __init__(self, kind):
        self.kind, self.g2 = kind, kind == 4
        self.G, self.gen, self.zero = (O.G2, O.G2_GEN, O.G2_ZERO) if self.g2 else (O.G1, O.G1_GEN, O.G1_ZERO)
        self.F = O.FQ2 if self.g2 else O.FQ
        self.cw = 2 * NL if self.g2 else NL

    def comps(self, e):
        return list(e) if self.g2 else [e]

    def elem(self, cs):
        return tuple(cs) if self.g2 else cs[0]

    def scale(self, e, lam_pow):
        return self.F.Mul(e, lam_pow)

    def one(self):
        return (1, 0) if self.g2 else 1

    def jac(self, aff):
        return self.zero if aff is None else (aff[0], aff[1], self.one())

    def coord_limbs(self, e, k):
        """Montgomery form of every component, shifted by k p, normal limbs"""
        return [v for c in self.comps(e) for v in normal_limbs(c * MONT_R % O.Q + k * O.Q)]

    def xyzz_limbs(self, aff, lam, shifts):
        if aff is None:
            return [0] * (4 * self.cw)
        F = self.F
        l2 = F.Mul(lam, lam)
        l3 = F.Mul(l2, lam)
        coords = (F.Mul(aff[0], l2), F.Mul(aff[1], l3), l2, l3)
        return [v for e, k in zip(coords, shifts) for v in self.coord_limbs(e, k)]

    def affine_limbs(self, aff):
        if aff is None:
            return [0] * (4 * self.cw)
        return self.coord_limbs(aff[0], 0) + self.coord_limbs(aff[1], 0) + [0] * (2 * self.cw)

    def rand_lam(self, rng):
        return (rng.randrange(1, O.Q), rng.randrange(O.Q)) if self.g2 else rng.randrange(1, O.Q)

    def ref_add(self, p, q):
        G = self.G
        if G.IsZero(p):
            return q
        if G.IsZero(q):
            return p
        ap, aq = G.Affine(p), G.Affine(q)
        if ap[0] == aq[0]:
            return G.Double(p) if ap[1] == aq[1] else self.zero       # the reference's Add has no P == Q branch (g1.go:32-89)
        return G.Add(p, q)


def point_plan(kind, seed):
    """{op: [(record words, expected affine or None, tag)]}: generic P + Q, P + P, P + (-P), infinity on either side, each with the
    accumulator's coordinates at v + k p for EVERY k its type admits -- the full product over (x, y, zz, zzz): 9 x 5 x 2 x 2 shift sets,
    9 x 2 x 2 x 2 for the tight accumulator, top set included -- so that P = U2 - X1 + 10 p and R vanish at every multiple of p they can
    take.  An XYZZ second operand walks the same product in another order.  (ZZ, ZZZ) alternate between (1, 1) and random."""
    cv, rng = Curve(kind), random.Random(seed)
    G = cv.G
    aff = lambda k: G.Affine(G.MulScalar(cv.gen, k))                              # noqa: E731
    neg = lambda a: None if a is None else G.Affine(G.Neg(cv.jac(a)))             # noqa: E731
    pts = [aff(rng.randrange(1, O.R)) for _ in range(3)] + [aff(1)]
    plan = {}
    for op, name in POINT_OPS.items():
        if name.startswith("tight") and not cv.g2:
            continue
        bounds = TIGHT_BOUNDS if name.startswith("tight") else XYZZ_BOUNDS
        shift_sets = list(itertools.product(*(range(b) for b in bounds)))
        operand_sets = list(itertools.product(*(range(b) for b in XYZZ_BOUNDS)))
        negate = name.endswith("negate")
        cases, seen = [], {}
        for tag in ("generic", "double", "cancel", "inf_acc", "inf_operand", "inf_both"):
            for j, sh in enumerate(shift_sets):
                P, Qo = pts[j % len(pts)], pts[(j + 1) % len(pts)]
                a, b = {"generic": (P, Qo), "double": (P, P), "cancel": (P, neg(P)), "inf_acc": (None, Qo), "inf_operand": (P, None),
                        "inf_both": (None, None)}[tag]
                lam_a, lam_b = (cv.one(), cv.one()) if j % 2 == 0 else (cv.rand_lam(rng), cv.rand_lam(rng))
                sh_b = operand_sets[(37 * j + 11) % len(operand_sets)]             # 37 is coprime to 180: every set once
                if name == "dbl":
                    want, second = (None if a is None else G.Affine(G.Double(cv.jac(a)))), [0] * (4 * cv.cw)
                else:
                    want = G.Affine(cv.ref_add(cv.jac(a), cv.jac(b)))
                    operand = neg(b) if negate else b                               # the op negates it back
                    second = cv.affine_limbs(operand) if "madd" in name else cv.xyzz_limbs(operand, lam_b, sh_b)
                cases.append((cv.xyzz_limbs(a, lam_a, sh) + second, want, "%s shift %s" % (tag, sh)))
                seen.setdefault(tag, set()).add(sh)
                if name in ("add", "add_mem"):
                    seen.setdefault(tag + " operand", set()).add(sh_b)
        top = tuple(b - 1 for b in bounds)
        for tag, shs in seen.items():                                             # every k of every coordinate, the top set included
            full = operand_sets if tag.endswith(" operand") else shift_sets
            assert shs == set(full) and (tuple(b - 1 for b in XYZZ_BOUNDS) if tag.endswith(" operand") else top) in shs, (name, tag)
        for rec, _, _ in cases:                                                   # the accumulator's (and an XYZZ operand's) declared type
            for base in ((0, 4 * cv.cw) if name in ("add", "add_mem") else (0,)):
                for c, b in enumerate(XYZZ_BOUNDS if base else bounds):
                    for h in range(cv.cw // NL):
                        at = base + c * cv.cw + h * NL
                        assert_fe(rec[at:at + NL], b, O.Q)
        plan[op] = cases
    return plan


def check_point_op(kind, op, cases, out):
    cv, q = Curve(kind), O.Q
    F = cv.F
    bounds = TIGHT_BOUNDS if POINT_OPS[op].startswith("tight") else XYZZ_BOUNDS
    rinv = pow(MONT_R, -1, q)
    for (rec, want, tag), o in zip(cases, out):
        o = [int(v) for v in o]
        what = "%s %s" % (POINT_OPS[op], tag)
        coords = []
        for c, b in enumerate(bounds):
            comp = [o[c * cv.cw + h * NL:c * cv.cw + (h + 1) * NL] for h in range(cv.cw // NL)]
            if any(o[2 * cv.cw:3 * cv.cw]):                                        # finite: every coordinate satisfies its declared type
                for limbs in comp:
                    assert_fe(limbs, b, q)
            coords.append(cv.elem([value(limbs) * rinv % q for limbs in comp]))
        if not any(o[2 * cv.cw:3 * cv.cw]):                                        # infinity <=> all limbs of zz are zero
            assert want is None, what + ": infinity"
            continue
        X, Y, ZZ, ZZZ = coords
        assert want is not None, what + ": should be infinity"
        assert F.Affine(ZZ) != F.Zero() and F.Affine(ZZZ) != F.Zero(), what + ": a finite point with ZZ or ZZZ == 0 (mod q)"
        assert F.Affine(F.Mul(F.Mul(ZZ, ZZ), ZZ)) == F.Affine(F.Mul(ZZZ, ZZZ)), what + ": ZZ^3 != ZZZ^2"
        got = (F.Affine(F.Mul(X, F.Inverse(ZZ))), F.Affine(F.Mul(Y, F.Inverse(ZZZ))))
        assert got == (F.Affine(want[0]), F.Affine(want[1])), what
