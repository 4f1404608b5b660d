"""gs_groth16_verify_each_keys against the per-key loop of gs_groth16_verify_each it replaces -- dev tool, two modes, one GPU.

    python tools/time_verify_each_keys.py old OUT.json
    python tools/time_verify_each_keys.py new PARENT.json [profiles/verify_each_keys_timing.txt] ["resource-usage lines of the kernels"]   (overwrites)

`old` uses only entry points the library had before this call existed (gs_g1_fixed_base, gs_g2_fixed_base, gs_groth16_verify_each), so
the same file runs in a checkout of the parent commit with that commit's library and binding; it writes its wall times as JSON.  `new`
times the new call in this tree and holds it against the parent's JSON.  Both build the same workload from the same seeds:

  A  64 known-log keys (npublic 3) with 16 valid proofs each, interleaved (proof i belongs to key i mod 64).  A = a G1, B = b G2,
     C = ((ab - alpha beta - gamma vkx) / delta) G1; all points come from gs_g1_fixed_base / gs_g2_fixed_base.
     old: the loop of 64 gs_groth16_verify_each calls, one per key, over the same proofs (sorted by key beforehand, not timed).
     new: ONE gs_groth16_verify_each_keys call over 64 prepared handles.
     Bound, set before any run: the one call takes at most 1/8 of the parent's loop.
  B  one such key, 4096 valid proofs.  old: one gs_groth16_verify_each call.  new: one gs_groth16_verify_each_keys call.
     Bound, set before any run: at most 1.10 x the parent's time.
  recorded without a bound (new): gs_groth16_vk_create per key, the device-time split (gs_last_timing), gs_groth16_verify per proof on
  the host for scale, 256 keys x 1 proof (every wave has one live lane), and the old entry point's loop and call in this tree's library.

Arguments are marshalled beforehand: a time is the wall time of the C call(s).  Medians of REPS after a warm-up of everything.  The last
argument is copied into the file: the register / LDS / scratch figures of the kernels from the code-object metadata, which this tool
cannot produce itself."""
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi  # noqa: E402

REPS, SAMPLE = 5, 64
R = capi.R
mode = sys.argv[1] if len(sys.argv) > 1 else "new"
assert mode in ("old", "new") and len(sys.argv) > 2, __doc__
capi.init()
med = statistics.median


class Keys:
    """nkeys known-log keys with npublic 3 and per[k] valid proofs each, as word arrays; everything from one seed."""

    def __init__(self, nkeys, per, seed):
        rng = random.Random(seed)
        self.nkeys, self.per = nkeys, per
        g1s, g2s, self.sig, self.kop = [], [], [], []
        secrets = []
        for _ in range(nkeys):
            al, be, ga, de = (rng.randrange(1, R) for _ in range(4))
            ics = [rng.randrange(1, R) for _ in range(4)]
            secrets.append((al, be, ga, de, ics))
            g1s += [al] + ics
            g2s += [be, ga, de]
        n = nkeys * per
        a_s, b_s, c_s = [], [], []
        for i in range(n):                                              # interleaved: proof i belongs to key i mod nkeys
            k = i % nkeys
            al, be, ga, de, ics = secrets[k]
            a, b = rng.randrange(1, R), rng.randrange(1, R)
            sig = [rng.randrange(R) for _ in range(3)]
            vkx = (ics[0] + sum(s * t for s, t in zip(sig, ics[1:]))) % R
            a_s.append(a)
            b_s.append(b)
            c_s.append((a * b - al * be - ga * vkx) * pow(de, R - 2, R) % R)
            self.sig.append(sig)
            self.kop.append(k)
        g1 = capi.g1_download(capi.g1_fixed_base(capi.ints_to_u64(g1s + a_s + c_s)))
        g2 = capi.g2_download(capi.g2_fixed_base(capi.ints_to_u64(g2s + b_s)))
        self.key_g1 = np.ascontiguousarray(g1[:5 * nkeys]).reshape(nkeys, 5, 12)          # alpha, IC_0 .. IC_3
        self.key_g2 = np.ascontiguousarray(g2[:3 * nkeys]).reshape(nkeys, 3, 24)          # beta, gamma, delta
        self.a = np.ascontiguousarray(g1[5 * nkeys:5 * nkeys + n])
        self.c = np.ascontiguousarray(g1[5 * nkeys + n:])
        self.b = np.ascontiguousarray(g2[3 * nkeys:])
        self.pub = capi.ints_to_u64([x for s in self.sig for x in s]).reshape(n, 12)
        self.n = n

    def key_args(self, k):
        ic = np.ascontiguousarray(self.key_g1[k, 1:])
        self._keep = getattr(self, "_keep", []) + [ic]
        return (capi.ptr64(self.key_g1[k, 0]), capi.ptr64(self.key_g2[k, 0]), capi.ptr64(self.key_g2[k, 1]), capi.ptr64(self.key_g2[k, 2]),
                capi.ptr64(ic), 4)

    def by_key(self):
        """per key: (pub, a, b, c) of its proofs, contiguous"""
        out = []
        for k in range(self.nkeys):
            at = [i for i in range(self.n) if self.kop[i] == k]
            out.append(tuple(np.ascontiguousarray(v[at]) for v in (self.pub, self.a, self.b, self.c)))
        return out


def old_each(key_args, pub, a, b, c):
    n = a.shape[0]
    ok, nbad = np.zeros(n, dtype=np.intc), ctypes.c_uint64(0)
    capi.call("gs_groth16_verify_each", *key_args, capi.ptr64(pub), 3, capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), n, ok.ctypes.data_as(capi.intp),
              ctypes.byref(nbad))
    assert nbad.value == 0 and ok.all()


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


many, one = Keys(64, 16, 41), Keys(1, 4096, 42)
many_args = [many.key_args(k) for k in range(64)]
many_sets = many.by_key()
one_args = one.key_args(0)


def old_loop():
    for k in range(64):
        old_each(many_args[k], *many_sets[k])


def old_one():
    old_each(one_args, one.pub, one.a, one.b, one.c)


if mode == "old":
    rows = {"loop": [], "one": []}
    for rep in range(REPS + 1):
        r = (timed(old_loop), timed(old_one))
        if rep:
            rows["loop"].append(r[0])
            rows["one"].append(r[1])
    res = {"loop_ms": med(rows["loop"]), "loop_all": rows["loop"], "one_ms": med(rows["one"]), "one_all": rows["one"], "version": capi.version()}
    with open(sys.argv[2], "w") as f:
        json.dump(res, f)
    print(json.dumps(res))
    sys.exit(0)

# ---- new ----------------------------------------------------------------------------------------------------------------------
with open(sys.argv[2]) as f:
    parent = json.load(f)
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "verify_each_keys_timing.txt")
resource = sys.argv[4] if len(sys.argv) > 4 else "(not given)"
PARTS = ("total_ms", "h2d_ms", "poly_ms", "plan_ms", "accumulate_ms", "reduce_ms")
sparse = Keys(256, 1, 43)


def create(ks, k):
    h = capi.Handle(0)
    capi.call("gs_groth16_vk_create", *ks.key_args(k), ctypes.byref(h))
    return capi.DeviceHandle(h.value)


create_ms = []
handles = {}
for name, ks in (("many", many), ("one", one), ("sparse", sparse)):
    hs = []
    for k in range(ks.nkeys):
        t = time.perf_counter()
        hs.append(create(ks, k))
        create_ms.append((time.perf_counter() - t) * 1e3)
    handles[name] = hs


def new_call(ks, hs):
    kop = np.array(ks.kop, dtype=np.uint32)
    harr = capi.harr(hs)
    ok, nbad = np.zeros(ks.n, dtype=np.intc), ctypes.c_uint64(0)

    def run():
        capi.call("gs_groth16_verify_each_keys", harr, len(hs), capi.ptr32(kop), capi.ptr64(ks.pub), capi.ptr64(ks.a), capi.ptr64(ks.b), capi.ptr64(ks.c),
                  ks.n, ok.ctypes.data_as(capi.intp), ctypes.byref(nbad))
        assert nbad.value == 0 and ok.all()
    return run


def with_split(f):
    ms = timed(f)
    tm = capi.last_timing()
    return (ms,) + tuple(tm[k] for k in PARTS)


def host_loop():
    ok = ctypes.c_int(0)
    t = time.perf_counter()
    for i in range(SAMPLE):
        capi.call("gs_groth16_verify", *many_args[many.kop[i]], capi.ptr64(many.pub[i]), 3, capi.ptr64(many.a[i]), capi.ptr64(many.b[i]), capi.ptr64(many.c[i]),
                  ctypes.byref(ok))
        assert ok.value == 1
    return (time.perf_counter() - t) * 1e3


calls = {"many": new_call(many, handles["many"]), "one": new_call(one, handles["one"]), "sparse": new_call(sparse, handles["sparse"])}
rows = {k: [] for k in ("many", "one", "sparse", "loop", "old_one", "host")}
for rep in range(REPS + 1):                                            # rep 0 warms everything up; the sides alternate
    r = {"many": with_split(calls["many"]), "loop": timed(old_loop), "one": with_split(calls["one"]), "old_one": timed(old_one),
         "sparse": with_split(calls["sparse"]), "host": host_loop()}
    if rep:
        for k, v in r.items():
            rows[k].append(v)


def split(name):
    return tuple(med([r[1 + k] for r in rows[name]]) for k in range(len(PARTS)))


wall = {k: med([r[0] for r in rows[k]]) for k in ("many", "one", "sparse")}
ratio_a, ratio_b = wall["many"] / parent["loop_ms"], wall["one"] / parent["one_ms"]
fmt = "      device %.2f ms: signals and tables up %.2f, membership %.2f, vkx %.2f, Miller %.2f, final exponentiation %.2f; wall - device %.2f"
lines = ["gs_groth16_verify_each_keys against the per-key loop of gs_groth16_verify_each at the parent commit's library (%s)" % parent.get("version", "?"),
         "known-log keys with 3 public inputs, valid proofs, points from gs_g*_fixed_base; wall time of the C call(s), medians of %d after a warm-up" % REPS,
         "  A  64 keys x 16 proofs, interleaved",
         "      parent, loop of 64 gs_groth16_verify_each calls  %9.2f ms   (%s)" % (parent["loop_ms"], "  ".join("%.2f" % v for v in parent["loop_all"])),
         "      ONE gs_groth16_verify_each_keys call             %9.2f ms   (%s)" % (wall["many"], "  ".join("%.2f" % r[0] for r in rows["many"])),
         fmt % (split("many") + (max(wall["many"] - split("many")[0], 0.0),)),
         "      bound, set before any run: one call <= 1/8 of the parent's loop (0.125): ratio %.4f (1/%.1f): %s"
         % (ratio_a, 1 / ratio_a, "MET" if ratio_a <= 0.125 else "NOT MET"),
         "      the same loop with this tree's library, same process: %.2f ms (recorded)" % med(rows["loop"]),
         "  B  one key x 4096 proofs",
         "      parent, one gs_groth16_verify_each call          %9.2f ms   (%s)" % (parent["one_ms"], "  ".join("%.2f" % v for v in parent["one_all"])),
         "      one gs_groth16_verify_each_keys call             %9.2f ms   (%s)" % (wall["one"], "  ".join("%.2f" % r[0] for r in rows["one"])),
         fmt % (split("one") + (max(wall["one"] - split("one")[0], 0.0),)),
         "      bound, set before any run: <= 1.10 x the parent's call: ratio %.3f: %s" % (ratio_b, "MET" if ratio_b <= 1.10 else "NOT MET"),
         "      gs_groth16_verify_each with this tree's library, same process: %.2f ms (recorded)" % med(rows["old_one"]),
         "  recorded, not bounded",
         "      gs_groth16_vk_create per key: median %.2f ms, worst %.2f ms over %d keys (host: curve tests, e(alpha, beta), two prepared lists)"
         % (med(create_ms), max(create_ms), len(create_ms)),
         "      gs_groth16_verify on the host: %.2f us / proof over %d proofs, one core" % (med(rows["host"]) / SAMPLE * 1e3, SAMPLE),
         "      256 keys x 1 proof (one live lane per wave)      %9.2f ms   (%s)" % (wall["sparse"], "  ".join("%.2f" % r[0] for r in rows["sparse"])),
         fmt % (split("sparse") + (max(wall["sparse"] - split("sparse")[0], 0.0),)),
         "  kernels, code-object metadata: %s" % resource, ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
