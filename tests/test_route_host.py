"""The prover's route decision (csrc/route.h: which h array a proof's h-sum runs against, and its lengths), instantiated on the
HOST (tests/host/route_host_test.hip) and compared, over the whole product of source kinds and key shapes, with a table written out
here from the rules.  Nothing below calls the library.  No GPU.

The rules, in their order:
  1. a values slice goes to the values route, and so does a witness when the evaluation-basis route is open;
  2. otherwise a coset-only key refuses;
  3. otherwise nh = len(px) - nz + 1 (0 when px is shorter than Z), and nh > len_h fails;
  4. the quotient-basis route: not the values route, not a witness over a nodes R1CS, a full key, nh >= 1, the key serves it, nh <= n_q;
  5. a key slice asked for another shard than its own fails;
  6. the range: a slice's own evaluation-basis range on the values route, else its own h range clipped to nh; a full key: the call's
     shard of nh.  hbase = where the first term sits in what the key holds.
"""
import itertools

import pytest

import hostbuild

KINDS = ["px_resident", "px_on_host", "px_from_r1cs", "witness", "values"]
NZ, LEN_H, N_EVAL = 5, 4, 4                        # Z of degree 4; 4 points in h; 4 constraints / a domain of 4 points
SHAPES = {"full": (0, 1), "slice0of3": (0, 3), "slice2of3": (2, 3)}
# the split of 4 terms over 3 shards is 2 + 1 + 1: what a key of each shape holds of a 4-term array
HELD = {"full": (0, 4), "slice0of3": (0, 2), "slice2of3": (3, 4)}
EVALS = ["nodes", "coset", "none"]
# len(px) -> len(hx) for nz = 5
QUOTIENT_LEN = {0: 0, 4: 0, 5: 1, 8: 4, 9: 5}
# (shape, nh) -> (hlo, hhi) of a px route: the held h range clipped to nh
PX_RANGE = {("full", 0): (0, 0), ("full", 1): (0, 1), ("full", 4): (0, 4),
            ("slice0of3", 0): (0, 0), ("slice0of3", 1): (0, 1), ("slice0of3", 4): (0, 2),
            ("slice2of3", 0): (0, 0), ("slice2of3", 1): (1, 1), ("slice2of3", 4): (3, 4)}


class Case:
    def __init__(self, kind, shape, evalb, has_quot, coset_only, npx, eval_open=None, nodes=None, call=None):
        self.kind, self.shape, self.evalb, self.has_quot, self.coset_only, self.npx = kind, shape, evalb, has_quot, coset_only, npx
        # a witness comes with the R1CS whose basis the key's array is: over the nodes unless the array is a coset basis
        self.eval_open = (evalb != "none") if eval_open is None else eval_open
        self.nodes = (evalb != "coset") if nodes is None else nodes
        self.call = SHAPES[shape] if call is None else call
        self.len_h = 0 if coset_only else LEN_H           # a coset-only key holds no monomial h array

    def line(self):
        index, count = SHAPES[self.shape]
        h_lo, h_hi = HELD[self.shape] if self.len_h else (0, 0)
        n_eval = 0 if self.evalb == "none" else N_EVAL
        e_lo, e_hi = HELD[self.shape] if n_eval else (0, 0)
        n_q = self.len_h if self.has_quot else 0
        nums = [KINDS.index(self.kind), self.npx, self.eval_open, self.nodes, NZ, self.len_h, index, count, h_lo, h_hi - h_lo,
                n_eval, e_lo, e_hi - e_lo, n_q, self.coset_only, n_q != 0, self.call[0], self.call[1]]
        return " ".join(str(int(x)) for x in nums)

    def skip(self):
        # the *_values fronts refuse a key without a nodes evaluation-basis array before the engine sees the call
        if self.kind == "values" and self.evalb != "nodes":
            return "values slice on a key without a nodes evaluation-basis array"
        return None

    def expected(self):
        sliced = self.shape != "full"
        on_values = self.kind == "values" or (self.kind == "witness" and self.eval_open)          # rule 1
        if not on_values and self.coset_only:
            return "err coset_only"                                                               # rule 2
        if on_values:
            nh = N_EVAL
        else:
            nh = QUOTIENT_LEN[self.npx]                                                           # rule 3
            if nh > self.len_h:
                return "err hx_too_long"
        quot = (not on_values and not (self.kind == "witness" and self.nodes) and not sliced and nh >= 1
                and self.has_quot and nh <= self.len_h)                                           # rule 4 (n_q = len_h)
        if sliced and self.call != SHAPES[self.shape]:
            return "err shard_mismatch"                                                           # rule 5
        if on_values:                                                                             # rule 6
            lo, hi = HELD[self.shape]
        elif self.call == (1, 3):                      # a full key asked for the middle shard of nh terms: 4 = 2 + [1] + 1, 1 = 1 + [0] + 0
            lo, hi = {4: (2, 3), 1: (1, 1), 0: (0, 0)}[nh]
        else:
            lo, hi = PX_RANGE[(self.shape, nh)]
        # what the key holds starts at the slice's first term (or before the clipped range): the range starts at offset 0 of it,
        # except where a full key is asked for a later shard
        hbase = lo if not sliced else 0
        return "ok %s %d %d %d %d" % ("values" if on_values else "quot" if quot else "hx", nh, lo, hi, hbase)


def product():
    for kind, shape, evalb, has_quot, coset_only in itertools.product(KINDS, SHAPES, EVALS, [True, False], [False, True]):
        len_h = 0 if coset_only else LEN_H
        for npx in [0, NZ - 1, NZ, NZ + len_h - 1, NZ + len_h]:
            yield Case(kind, shape, evalb, has_quot, coset_only, npx)


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("route_host_test")


def check(exe, cases):
    got = hostbuild.run_lines(exe, [c.line() for c in cases])
    wrong = [(c.line(), c.expected(), g) for c, g in zip(cases, got) if g != c.expected()]
    assert not wrong, "%d of %d differ; first: %r" % (len(wrong), len(cases), wrong[:3])


def test_route_over_the_whole_product_of_sources_and_keys(exe):
    cases = list(product())
    assert len(cases) == 5 * 3 * 3 * 2 * 2 * 5
    kept = [c for c in cases if c.skip() is None]
    assert {c.skip() for c in cases} == {None, "values slice on a key without a nodes evaluation-basis array"}
    assert 4 * (len(cases) - len(kept)) < len(cases)          # under a quarter skipped (120 of 900)
    check(exe, kept)
    outcomes = {c.expected().split()[1] for c in kept}
    assert outcomes == {"values", "quot", "hx", "coset_only", "hx_too_long"}      # every route and both refusals occur


def test_route_cases_beside_the_product(exe):
    extra = []
    for has_quot in (True, False):
        for npx in (0, 4, 5, 8, 9):
            # a domain-R1CS witness whose evaluation-basis route is closed falls to px: quotient basis when the key has it
            extra.append(Case("witness", "full", "coset", has_quot, False, npx, eval_open=False, nodes=False))
            extra.append(Case("witness", "full", "none", has_quot, False, npx, eval_open=False, nodes=False))
            # a nodes-R1CS witness with the route closed although the key has the array (gs_set_eval_basis(0), the exact-route retry)
            extra.append(Case("witness", "full", "nodes", has_quot, False, npx, eval_open=False, nodes=True))
            # a full key asked for shard 1 of 3 (gs_*_prove_partials on a replicated key)
            extra.append(Case("px_resident", "full", "none", has_quot, False, npx, call=(1, 3)))
    # a key slice asked for another shard than its own, on either kind of route; a too-long px is reported first
    extra.append(Case("px_resident", "slice0of3", "nodes", False, False, 8, call=(1, 3)))
    extra.append(Case("px_resident", "slice2of3", "nodes", False, False, 9, call=(0, 1)))
    extra.append(Case("values", "slice2of3", "nodes", False, False, 0, call=(0, 3)))
    extra.append(Case("px_on_host", "slice0of3", "none", False, False, 5, call=(0, 1)))
    check(exe, extra)
    assert [c.expected() for c in extra[-4:]] == ["err shard_mismatch", "err hx_too_long", "err shard_mismatch", "err shard_mismatch"]
    assert Case("witness", "full", "coset", True, False, 8, eval_open=False, nodes=False).expected() == "ok quot 4 0 4 0"
    assert Case("witness", "full", "nodes", True, False, 8, eval_open=False, nodes=True).expected() == "ok hx 4 0 4 0"
    assert Case("px_resident", "full", "none", False, False, 8, call=(1, 3)).expected() == "ok hx 4 2 3 2"
