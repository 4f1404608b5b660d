"""The window tables' instalment schedule, call by call -- dev tool.
    python tools/table_schedule_trace.py          (GS_LIB=<another build of the library> to trace that one)
The schedule has no clock in it (the build credit is a function of term counts: csrc/tables.h, build_credit), so two builds of the
library that schedule alike print the same bytes.  Default knobs, policy auto, one line per call:
    <sequence> <call> <table bytes held by the handle> <gs_timing.window_bits> <evictions so far>
for a fresh 2^17 key proved 14 times; the same key through release_tables, three proofs, build_tables(., 1) and one proof; and a
150000-point G1 and a 150000-point G2 base array through 8 blocking MSMs each."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gosnark_amd  # noqa: E402,F401
from gosnark_amd import capi, groth16, synth  # noqa: E402

capi.init()
capi.set_table_policy("auto")


def line(seq, call, handle):
    print(seq, call, capi.handle_bytes(handle)[1], capi.last_timing()["window_bits"], capi.memory_query()["evictions"], flush=True)


inst = synth.sqchain_setup_instance(1 << 17, 0x7AB1)
pk = inst.device_pk()
r, s = synth.field_elems(2, 0x7AB)
first = groth16.prove_resident(pk, inst.w, inst.px, r, s)


def prove(seq, call):
    p = groth16.prove_resident(pk, inst.w, inst.px, r, s)
    assert (p.PiA, p.PiB, p.PiC) == (first.PiA, first.PiB, first.PiC), (seq, call)
    line(seq, call, pk.handle)


line("fresh_key", 0, pk.handle)
for i in range(1, 14):
    prove("fresh_key", i)
capi.release_tables(pk.handle)
line("released_key", "release", pk.handle)
for i in range(3):
    prove("released_key", i)
capi.build_tables(pk.handle, 1)
line("released_key", "build", pk.handle)
prove("released_key", 3)

for g2 in (False, True):
    m = 150000
    bases = (capi.g2_fixed_base if g2 else capi.g1_fixed_base)(synth.scalars_u64(m, 0x7AB2 + g2))
    sc = synth.scalars_u64(m, 0x7AB4 + g2)
    want = None
    for i in range(8):
        got = capi.msm(bases, sc, g2=g2)
        want = want or got
        assert got == want, (g2, i)
        line("g2_bases" if g2 else "g1_bases", i, bases)
