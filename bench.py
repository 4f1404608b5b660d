#!/usr/bin/env python
"""bench.py -- Groth16 prove throughput (constraints/s) of the HIP prover on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--reps R] [--log2n 20]
                    [--workload prove|prove_from_r1cs|prove_sharded|prove_pinocchio|msm_g1|msm_sharded] [--logical-shards S]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps once and prints the line: every check and every figure that needs runs of
its own (proof checks, the extras below, CPU baselines, the strong-scaling section, repetitions) is taken with --full only.
--dump-outputs DIR writes the last timed step's result (the proof's points, or the MSM's point) as DIR/<name>.npy; the inputs
are seeded, so two builds given the same arguments can be compared array by array.

A "step" is one full groth16.GenerateProofs (groth16/groth16.go:225-278: H(x) = P(x)/Z(x), the
five MSMs, the O(1) tail) over a synthetic instance with n = 2^log2n constraints, m = n + 1
variables, NPublic = 1 (BASELINE.json configs[2]); the proving key, w and px are resident in HBM
before the timed region.  The timed region (K steps between barrier + synchronize) is repeated R
times (R = 1, or 5 with --full); `ms_per_step` / `value` are the MEDIAN repetition, every repetition is listed.

N > 1 starts however it is invoked:
  * under torch.distributed.run (WORLD_SIZE = N in the environment): one rank per GPU; the control plane (barriers, the max over
    ranks, the communicator's unique id) runs on gloo, RCCL carries the data plane (the strong section's in-library communicator,
    ncclCommInitRank + ncclAllGather + ncclSend/ncclRecv, and a torch nccl-group all_reduce probe) AFTER the weak-scaling line is parked
    in the watchdog, so no RCCL problem of a first multi-GPU run can take the line with it;
  * plainly -- `python bench.py --gpus N` -- ONE process drives the N devices through the library's own multi-device
    entry points (gs_init(devs, N), gs_groth16_prove_batch, gs_groth16_prove_multi[_values], gs_msm_g1_multi; the
    records travel through the communicator of gs_comm_init_local = ncclCommInitAll, created after the weak-scaling line is parked).  With fewer than N GPUs visible
    the N devices are logical devices spread over the visible ones (and the line says so); `--multi ranks` re-executes
    the same command line under torch.distributed.run instead.
Either way `value` is the WEAK-scaling figure: every GPU proves independent instances of the same circuit with its own
witness (the batch-of-proofs partition of BASELINE.json configs[4]; no data-path collective), N * n * K / (max time);
and with --full the SAME line carries the STRONG-scaling figures under `strong` -- ONE 2^log2n proof whose MSM term ranges are split
over the N GPUs (both routes: replicated H(x) / owner's values scattered) and ONE 2^22-term G1 MSM split the same way
(BASELINE configs[3]), each checked against the single-device result / the naive-loop golden -- plus `rccl` (ranks the
communicator saw, mode, collectives executed) and `devices` (ordinals, hipDeviceCanAccessPeer matrix).
`--workload prove_sharded / msm_sharded` shards ONE proof / ONE G1 MSM across the ranks and gathers the
partial points INSIDE the library over RCCL (gs_groth16_prove_sharded / gs_msm_g1_sharded; configs[3],
SURVEY 8e).  With `--logical-shards S` on ONE GPU the S shards run as S logical devices of one process
(gs_groth16_prove_multi / gs_msm_g1_multi): per-shard times are measured and an S-GPU figure is MODELLED
from them (labelled as such) -- there is no multi-GPU hardware behind a gpurun call.

Prints ONE JSON line on rank 0, including
  roofline:     the dominant kernel (G1 bucket accumulation) against the HBM roofline,
  cpu_baseline: the reference algorithm (oracle/gs_oracle.c: naive MulScalar/Add loops + schoolbook
                Div) timed on ONE host core on a bounded sample (rank 0, N = 1, --full only),
and, on the single-GPU run with --full, the second half of BASELINE's metric (G1-MSM terms/s at 2^20 and
2^16), the blocking-call latency, witness -> proof from the resident sparse R1CS, the host-buffer
entry point, and the reference's own compiled prover (wasm under node) on a small instance.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, synth

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
MAD_PEAK_T = 34.4              # T lane-mad/s, v_mad_u64_u32 on 8 chains, 3 waves per SIMD, whole chip, SUSTAINED (4 s of launches at sclk 2.39 GHz: 4.47
                               # cycles per instruction per SIMD; tools/ubench_issue.hip 0 4 -> profiles/r06_power_clock_trace.txt).  Rounds 1-5 used 31.5, from
                               # a single launch out of idle, i.e. on a clock still ramping (2.1 GHz by s_memtime / s_memrealtime)
MAD_PIPE_T = 1024 * 16 * 2.4e9 / 1e12   # T lane-mad/s: the multiplier pipe, sixteen lanes per clock per SIMD (v_mad_u64_u32 and v_fma_f64 alike: the data sheet's FP64 vector peak)
G1_TERM_BYTES = 96             # 32 B scalar + 64 B affine base per G1 MSM term
MADS_PER_MIXED_ADD = 1467      # 6 products (162 mads) + 2 squarings (126) + one two-term product (243)
VALU_PER_MIXED_ADD = 2090      # SQ_INSTS_VALU per G1 mixed addition (profiles/r03_/r04_pmc_sq_accumulate_prove.txt)
# What bounds the dominant kernel (round 6, profiles/r06_power_clock_trace.txt -- which withdraws round 5's "3.15 real cycles per multiply-add at
# 1.2-1.35 GHz": a SIMD issues oldest-first, so the MEAN wave span round 5 divided by all three waves' instructions covers 70 % of the
# time they were issued in, and mean span / kernel time is not a clock; s_memtime ticks at sclk, 2.38-2.40 GHz in every sustained loop).
# Cycles per wave64 instruction per SIMD on the whole chip: v_mad_u64_u32 4.47, the other VOP3 / multiplier classes 4.4-4.8, VOP2 2.9,
# s_nop 1.35 -- and the SAME on a stream confined to 8 / 32 / 128 CUs (profiles/r06_ubench_placement_cu_mask.txt, which corrects a first
# reading of masked runs as a socket-level throttle: that mask did not confine the waves): it is the pipe's own rate, sixteen lanes per
# clock = 4 cycles per wave for the 64-bit / multiplier classes (the data sheet's FP64 vector peak), of which three waves per SIMD reach
# 89 %.  The socket draws 0.95-1.37 kW of its 1.4 kW cap in these loops; the PLL only drops in the real workloads.  fp29.h's own products (dots3, random data)
# run at 876 cycles per product per SIMD = 4.23 per VALU instruction: 745 200 VALU instructions per SIMD per 1.357 ms launch in a sustained
# loop.  That rate, chip-wide, is the peak below.
ISSUE_PEAK_G = 1024 * 0.5492   # G wave-instructions/s: 1024 SIMDs x 549.2 M/s (the dots3 product loop, sustained; round 5: 463 from a one-shot launch)
R = groth16.R


def checker_leg_proof(proof, inst, r_, s_, w_host=None):
    """Checker leg (with cpu_baseline below the only users of oracle/ in this file; never inside the timed region):
    PiA, PiB, PiC of the benchmarked instance against a*G1, b*G2, c*G1 computed by the C oracle's MulScalar from the
    closed-form scalars of synth.SqchainSetupInstance.expected_proof_scalars (w_host: another witness of the same circuit)."""
    from oracle import c_oracle as C, ref_py as O
    ea, eb, ec = inst.expected_proof_scalars(r_, s_, w_host)
    ok = ((proof.PiA[0], proof.PiA[1]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, ea)) and
          (proof.PiB[0], proof.PiB[1]) == C.g2_affine(C.g2_mul_scalar(O.G2_GEN, eb)) and
          (proof.PiC[0], proof.PiC[1]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, ec)))
    if not ok:
        raise SystemExit("bench.py: the proof of the benchmarked instance does not match its closed form")
    return "PiA, PiB, PiC equal a*G1, b*G2, c*G1 for the closed-form (a, b, c) derived from the setup's toxic values"


def cpu_baseline_all_cores(log2n_sample, seed):
    """Same algorithm with the term ranges of every MSM split over all host threads (oracle_msm_naive_mt); the reference
    itself is single-threaded (no goroutines), so this is an upper bound on what its algorithm gets from the host."""
    from oracle import c_oracle as C
    threads = os.cpu_count() or 1
    n = 1 << log2n_sample
    inst = synth.random_instance(n, seed)
    g1 = {k: capi.g1_download(inst.g1[k]) for k in ("at", "bacgamma", "bacdelta", "ptd")}
    g2 = capi.g2_download(inst.g2_bacgamma)
    w, hx = inst.w_host, inst.px_host[:n]          # the O(n^2) schoolbook Div is left out here (it does not thread)
    t0 = time.perf_counter()
    C.g1_msm_naive(g1["at"], w, threads=threads)
    C.g1_msm_naive(g1["bacgamma"], w, threads=threads)
    C.g2_msm_naive(g2, w, threads=threads)
    C.g1_msm_naive(g1["bacdelta"][2:], w[2:], threads=threads)
    C.g1_msm_naive(g1["ptd"], hx, threads=threads)
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "constraints/s", "cores": threads, "kind": "port",
            "sample": "the five naive MSMs of a Groth16 prove at n=2^%d (no Div), term ranges over %d threads, %.2f s" % (log2n_sample, threads, dt)}


def cpu_baseline(log2n_sample, seed):
    """The reference algorithm on one host core: sum_i MulScalar(base_i, w_i) loops
    (groth16.go:243-250,269-271 / g1.go:140-155 + :32-89) and schoolbook Div (r1csqap.go:70-84),
    via oracle/gs_oracle.c, on an instance with 2^log2n_sample constraints."""
    from oracle import c_oracle as C            # checker/baseline only; never on the product path
    n = 1 << log2n_sample
    inst = synth.random_instance(n, seed)       # device arrays -> downloaded Jacobian copies for the CPU
    g1 = {k: capi.g1_download(inst.g1[k]) for k in ("at", "bacgamma", "bacdelta", "ptd")}
    g2 = capi.g2_download(inst.g2_bacgamma)
    w, px, z = inst.w_host, inst.px_host, inst.z_host
    t0 = time.perf_counter()
    hx, _ = C.poly_div_u64(px, z)
    C.g1_msm_naive(g1["at"], w)
    C.g1_msm_naive(g1["bacgamma"], w)
    C.g2_msm_naive(g2, w)
    C.g1_msm_naive(g1["bacdelta"][2:], w[2:])
    C.g1_msm_naive(g1["ptd"][:hx.shape[0]], hx)
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "constraints/s", "cores": 1, "kind": "port",
            "sample": "full Groth16 prove at n=2^%d constraints (4 G1 + 1 G2 naive double-and-add MSMs of ~n terms "
                      "+ schoolbook Div), oracle/gs_oracle.c, 1 thread, %.1f s" % (log2n_sample, dt)}


def cpu_baseline_reference_wasm():
    """The reference's OWN code beside the GPU (BASELINE.md plan 2a): its compiled prover wasm/go-snark.wasm (go1.12 js/wasm build
    of groth16.GenerateProofs) under node, on the m = 17 instance of tests/golden/wasm_groth_rand_m17.json, checked to return the
    recorded proof.  oracle/_ref/go-snark.wasm is a copy made by `make -C oracle ref` in the build container (it travels to the
    GPU box with the snapshot; /root/reference does not exist there).  wasm on a JS engine is several times slower than native
    Go, hence the flag; larger instances are out of reach (Div is O(n^3): 39 s at n = 256)."""
    wasm = os.path.join(ROOT, "oracle", "_ref", "go-snark.wasm")
    node = shutil.which("node")
    if not (os.path.exists(wasm) and node):
        return {"skipped": "oracle/_ref/go-snark.wasm or node not available"}
    with open(os.path.join(ROOT, "tests", "golden", "wasm_groth_rand_m17.json")) as f:
        rec = json.load(f)
    job = [{"name": "bench", "kind": "groth", "circuit": rec["circuit"], "setup": rec["setup"], "px": rec["px"], "inputs": rec["inputs"],
            "rand": rec["rand"], "verify": []}]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "jobs.json"), "w") as f:
            json.dump(job, f)
        run = subprocess.run([node, os.path.join(ROOT, "oracle", "ref_wasm", "run_jobs.js"), wasm, os.path.join(d, "jobs.json"),
                              os.path.join(d, "out.json")], capture_output=True, text=True, timeout=300)
        if run.returncode != 0:
            return {"skipped": "node failed: " + run.stderr[-200:]}
        with open(os.path.join(d, "out.json")) as f:
            out = json.load(f)[0]
    n = json.loads(rec["circuit"])["NVars"] - 1
    if out["proof"] != rec["proof"]:
        return {"skipped": "the wasm prover did not reproduce the recorded proof"}
    ver = subprocess.run([node, "--version"], capture_output=True, text=True).stdout.strip()
    return {"value": n / (out["prove_ms"] / 1e3), "unit": "constraints/s", "cores": 1, "kind": "reference",
            "flag": "wasm under node %s (not native Go: no Go toolchain in the image)" % ver,
            "sample": "groth16.GenerateProofs of the reference (wasm/go-snark.wasm) at n = %d constraints (m = %d), %.2f s, proof equal to "
                      "tests/golden/wasm_groth_rand_m17.json" % (n, n + 1, out["prove_ms"] / 1e3)}


def witness_digit_stats(w_u64, c, tm):
    """What the MSM plan sees in a witness (host restatement of k_digits' signed-digit recoding, msm_kernels.h next_digit): the share
    of zero digits (skipped: no bucket addition), the heaviest bucket, and the buckets the plan cuts into more than 64 chunks
    (k_heavy_combine's block-wide tree).  Uniform 254-bit scalars: zero share 2^-c, every bucket ~ n W / 2^(c-1) entries."""
    w = np.ascontiguousarray(w_u64, dtype=np.uint64).reshape(-1, 4)
    n = w.shape[0]
    W, B = 254 // c + 1, 1 << (c - 1)
    carry = np.zeros(n, dtype=np.int64)
    counts = np.zeros(B + 1, dtype=np.int64)
    zeros = 0
    for win in range(W):
        lo = win * c
        word, off = lo // 64, lo % 64
        raw = (w[:, word] >> np.uint64(off)).astype(np.uint64)
        if off + c > 64 and word + 1 < 4:
            raw |= w[:, word + 1] << np.uint64(64 - off)
        raw = (raw & np.uint64((1 << c) - 1)).astype(np.int64) + carry
        carry = (raw > B).astype(np.int64)
        d = np.abs(raw - carry * 2 * B)
        zeros += int((d == 0).sum())
        counts += np.bincount(d, minlength=B + 1)
    entries = int(counts[1:].sum())
    chunk = 32 if entries >= (1 << 23) else 16          # msm.hip choose_chunk (before its heavy-bucket growth)
    return {"window_bits": c, "digits": n * W, "zero_digit_share": zeros / float(n * W), "bucket_additions_per_base_array": entries,
            "heaviest_bucket_entries": int(counts[1:].max()), "median_bucket_entries": float(np.median(counts[1:])),
            "buckets_cut_into_more_than_64_chunks": int((counts[1:] > 65 * chunk).sum()),
            "gs_timing_of_the_last_proof": {k: tm.get(k) for k in ("plan_digits", "plan_entries", "heavy_buckets")},
            "note": "host restatement of the plan's digit recoding over the witness (the sums over w: 4 of the 5 MSMs), beside what the plans themselves "
                    "counted on the device for the last proof (gs_timing: all five sums, the uniform h-scalars included); acc_*_adds and roofline_valu "
                    "count the non-zero digits only"}


def cpus_granted():
    """What the container really gives this process (os.cpu_count() reports the host's threads): the scheduler affinity and the cgroup
    CPU quota, so that `cpu_baseline_all_cores` can be read for what it is."""
    info = {"os_cpu_count": os.cpu_count()}
    try:
        info["sched_affinity"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
            if path.endswith("cpu.max"):
                info["cgroup_quota_cpus"] = None if txt[0] == "max" else float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0])
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                    info["cgroup_quota_cpus"] = None if q < 0 else q / float(g.read())
            break
        except (OSError, ValueError, IndexError):
            continue
    return info


def stream_distinct_host(inst, pk, n, r_, s_, distinct=8, steps=16, reps=3, check=True):
    """the reference's call shape at the pipelined rate.  `distinct` different satisfying witnesses of the
    benchmarked circuit rotate; every step brings ANOTHER one in pageable host memory (groth16.GenerateProofs gets a fresh w -- and
    px -- per call, groth16/groth16.go:225, cli/main.go:480-501); three proofs in flight.  Four ways in, each timed:
      witness_host   gs_groth16_prove_witness_host_begin (32 MiB per proof at 2^20; the slot's own device buffers, copy stream)
      px_host        gs_groth16_prove_host_begin (w and px: 96 MiB per proof)
      update         gs_scalars_update into four rotating resident vectors + gs_groth16_prove_witness_begin
      resident       the same rotation with every witness uploaded beforehand (the figure the others are compared with)
    Afterwards (outside every timed region) each of the `distinct` proofs of the witness_host stream is checked against ITS closed
    form from the setup's toxic values and by groth16.VerifyProof against ITS public input (and rejected for another's)."""
    from gosnark_amd import r1csqap
    dr = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
    xs = synth.field_elems(distinct, inst.seed + 9000)
    ws = [synth.sqchain_witness(n, x) for x in xs]                      # plain numpy arrays: pageable host memory
    w_res = [capi.scalars_upload(w) for w in ws]
    pxs = []
    for h in w_res:                                                     # px of every witness, back in host memory
        ph = dr.ComputePxResident(h)
        pxs.append(capi.scalars_download(ph))
        ph.free()
    rot = [capi.scalars_upload(ws[k]) for k in range(4)]
    proofs = {}

    def run(begin_k, count, keep=None):
        tickets = []
        for i in range(count):
            k = i % distinct
            tickets.append((k, begin_k(k, i)))
            if len(tickets) == 3:
                kk, t = tickets.pop(0)
                p = groth16.prove_end(t)
                if keep is not None:
                    keep[kk] = p
        while tickets:
            kk, t = tickets.pop(0)
            p = groth16.prove_end(t)
            if keep is not None:
                keep[kk] = p

    def upd(k, i):
        capi.scalars_update(rot[i % 4], ws[k])
        return groth16.prove_witness_begin(pk, dr, rot[i % 4], r_, s_)
    modes = {
        "witness_host": lambda k, i: groth16.prove_witness_host_begin(pk, dr, ws[k], r_, s_),
        "px_host": lambda k, i: groth16.prove_host_begin(pk, ws[k], pxs[k], r_, s_),
        "update": upd,
        "resident": lambda k, i: groth16.prove_witness_begin(pk, dr, w_res[k], r_, s_),
        "px_resident_same_witness": lambda k, i: groth16.prove_begin(pk, inst.w, inst.px, r_, s_),
    }
    out = {"distinct_witnesses": distinct, "steps_per_repetition": steps, "proofs_in_flight": 3,
           "bytes_per_proof": {"witness_host": int(ws[0].nbytes), "px_host": int(ws[0].nbytes + pxs[0].nbytes)}}
    for name, fn in modes.items():
        run(fn, 2 * distinct, proofs if name == "witness_host" else None)      # warm: the slots' buffers exist after the first lap
        a0 = capi.alloc_counters()
        samples = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(fn, steps)
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) / steps * 1e3)
        a1 = capi.alloc_counters()
        out[name] = {"ms_per_proof": statistics.median(samples), "ms_per_proof_reps": samples, "constraints_per_s": n / statistics.median(samples) * 1e3,
                     "hipMalloc_calls_in_timed_steps": a1[0] - a0[0], "hipFree_calls_in_timed_steps": a1[1] - a0[1]}
    out["witness_host_over_resident"] = out["witness_host"]["ms_per_proof"] / out["resident"]["ms_per_proof"]
    out["px_host_over_px_resident"] = out["px_host"]["ms_per_proof"] / out["px_resident_same_witness"]["ms_per_proof"]
    if check:
        ok_v = 0
        for k in range(distinct):
            p = proofs[k]
            checker_leg_proof(p, inst, r_, s_, ws[k])                   # raises SystemExit on a mismatch
            if groth16.VerifyProof(inst.vk, p, [xs[k]]) and not groth16.VerifyProof(inst.vk, p, [xs[(k + 1) % distinct]]):
                ok_v += 1
        if ok_v != distinct:
            raise SystemExit("bench.py: groth16.VerifyProof rejected a proof of the distinct-witness stream (%d of %d accepted)" % (ok_v, distinct))
        out["checked"] = ("each of the %d streamed proofs equals the closed form of ITS witness (toxic values of the setup) and is accepted by "
                          "groth16.VerifyProof for its own public input and rejected for its neighbour's" % distinct)
    for h in w_res + rot:
        h.free()
    dr.handle.free()
    return out


def cold_path(inst, pk, n, r_, s_, ref_proof):
    """the reference's other call shape -- load a key, prove ONCE (cli/main.go:330-349).  The resident key is
    written to a binary key file and loaded back (np.memmap -> gs_g1_upload / gs_g2_upload -> gs_groth16_pk_create: what a CLI does);
    `cold_ms` = gs_groth16_pk_create (+ gs_groth16_pk_set_eval) -> first proof collected, the uploads are given beside it.  Under
    table policy `auto` the first proof is summed table-free; under `always` (rounds 1-4) it first builds 5.6 GiB of window tables."""
    import tempfile
    from gosnark_amd import utils
    path = os.path.join(tempfile.gettempdir(), "gs_cold_key_%d.bin" % os.getpid())
    utils.GrothSetupToBinary(path, groth16.Circuit(pk.nvars, pk.npublic), pk, None)
    out = {"key_file_bytes": os.path.getsize(path)}
    try:
        def fresh_key(policy):
            """One load of the key file -> the first proofs of that key under `policy`; everything it uploaded is freed again."""
            out = {}
            capi.set_table_policy(policy)
            protocol, nvars, npublic, sec = utils.ReadBinary(path)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            up1 = lambda k: capi.g1_upload(np.ascontiguousarray(sec[k], dtype=np.uint64))     # noqa: E731
            at, b1, cd, pt = up1("G1.At"), up1("G1.BACGamma"), up1("BACDelta"), up1("PowersTauDelta")
            b2 = capi.g2_upload(np.ascontiguousarray(sec["G2.BACGamma"], dtype=np.uint64))
            ev = up1("PowersTauDeltaEval") if "PowersTauDeltaEval" in sec else None
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            abd, bd = utils._g1_tuples(sec["G1.ABD"]), utils._g2_tuples(sec["G2.BD"])
            k2 = groth16.device_pk_from_handles(at, b1, b2, cd, pt, abd[0], abd[1], abd[2], bd[0], bd[1], np.ascontiguousarray(sec["Z"], dtype=np.uint64),
                                                nvars, npublic)
            if ev is not None:
                capi.check(capi.load_library().gs_groth16_pk_set_eval(capi.Handle(k2.handle.h), capi.Handle(ev.h)))
            t2 = time.perf_counter()
            p = groth16.prove_resident(k2, inst.w, inst.px, r_, s_)
            t3 = time.perf_counter()
            if (p.PiA, p.PiB, p.PiC) != (ref_proof.PiA, ref_proof.PiB, ref_proof.PiC):
                raise SystemExit("bench.py: the first proof of the freshly loaded key (table policy %s) differs from the warm key's" % policy)
            obj_b, tab_b = capi.handle_bytes(k2.handle)
            p2 = groth16.prove_resident(k2, inst.w, inst.px, r_, s_)
            t4 = time.perf_counter()
            out[policy] = {"cold_ms": (t3 - t1) * 1e3, "pk_create_ms": (t2 - t1) * 1e3, "first_proof_ms": (t3 - t2) * 1e3, "second_proof_ms": (t4 - t3) * 1e3,
                           "key_upload_ms": (t1 - t0) * 1e3, "key_bytes_after_first_proof": obj_b, "table_bytes_after_first_proof": tab_b,
                           "first_proof_equals_warm_key": True, "second_proof_equals": (p2.PiA, p2.PiB, p2.PiC) == (p.PiA, p.PiB, p.PiC)}
            if policy == "auto":
                # Round 6: the whole transient of the fresh key -- blocking proofs back to back until the instalments are
                # through (msm.hip, prepare_tables: every call builds a few slabs of the pending tables in front of its own accumulations and
                # the call that enqueues the last slab switches over) -- then the steady state on the tables `auto` built
                ms, widths = [(t3 - t2) * 1e3, (t4 - t3) * 1e3], [None, capi.last_timing()["window_bits"]]
                t_prev = t4
                for _ in range(46):
                    q = groth16.prove_resident(k2, inst.w, inst.px, r_, s_)
                    t_now = time.perf_counter()
                    ms.append((t_now - t_prev) * 1e3); widths.append(capi.last_timing()["window_bits"]); t_prev = t_now
                    if (q.PiA, q.PiB, q.PiC) != (p.PiA, p.PiB, p.PiC):
                        raise SystemExit("bench.py: a proof of the key's warm-up transient differs from its first proof")
                free_w = widths[1]
                first_tabled = next((i for i, wdt in enumerate(widths) if wdt is not None and wdt != free_w), None)
                steady = statistics.median(ms[first_tabled + 2:]) if first_tabled is not None and first_tabled + 4 < len(ms) else None
                out[policy]["proofs_ms"] = [round(x, 2) for x in ms[:max(24, (first_tabled or 0) + 4)]]
                out[policy]["first_proof_on_tables"] = first_tabled
                out[policy]["steady_blocking_ms"] = steady
                out[policy]["time_to_steady_ms"] = (t2 - t1) * 1e3 + sum(ms[:first_tabled + 1]) if first_tabled is not None else None
                out[policy]["slowest_proof_after_the_first_over_steady"] = max(ms[1:]) / steady if steady else None
                out[policy]["note"] = ("blocking proofs back to back on a freshly loaded key: [0] table-free, then every call pays an instalment of the window "
                                       "tables (~125 ms of full-chip work per 2^20 key in all) until they serve; time_to_steady_ms counts from gs_groth16_pk_create. "
                                       "No schedule can have both `no proof above 2x steady` and `steady within 170 ms`: 24 ms + 125 ms of builds leave room for two "
                                       "table-free proofs before 170 ms, which would then take ~70 ms each (GS_TABLE_BUDGET_PCT moves along that line: "
                                       "profiles/r06_auto_instalments.txt)")
                samples = []
                pipelined(lambda: groth16.prove_begin(k2, inst.w, inst.px, r_, s_), groth16.prove_end, 6, 3)
                for _ in range(3):
                    torch.cuda.synchronize()
                    ta = time.perf_counter()
                    pipelined(lambda: groth16.prove_begin(k2, inst.w, inst.px, r_, s_), groth16.prove_end, 10, 3)
                    torch.cuda.synchronize()
                    samples.append((time.perf_counter() - ta) / 10 * 1e3)
                out[policy]["converged_pipelined_ms_per_proof"] = statistics.median(samples)
                out[policy]["converged_pipelined_reps"] = samples
            for h in (at, b1, cd, pt, b2) + ((ev,) if ev is not None else ()):
                h.free()
            k2.handle.free()
            del sec
            return out[policy]

        # the `auto` transient twice, on two fresh loads: its first calls allocate (workspaces of the table-free route, then 5.4 GiB of pending
        # tables), and hipMalloc on a shared node is now and then 5-10x slower than usual (one call of round 6: 52 and 208 ms for the first two
        # proofs instead of 23 and 18, the `always` load right after it as usual).  Both runs are in the line; the top-level fields are those of
        # the run whose slowest proof after the first is the shorter one.
        import gc

        def quiet_fresh_key(policy):
            # a fresh key on a quiet device and a quiet interpreter: let the driver finish with the gigabytes the previous measurement freed,
            # and keep Python's collector (this process holds millions of objects by now) out of the timed calls
            gc.collect()
            time.sleep(1.0)
            gc.disable()
            try:
                return fresh_key(policy)
            finally:
                gc.enable()
        runs = [quiet_fresh_key("auto"), quiet_fresh_key("auto")]
        key = lambda r_: (r_.get("slowest_proof_after_the_first_over_steady") or 1e9)     # noqa: E731
        best, other = (runs[0], runs[1]) if key(runs[0]) <= key(runs[1]) else (runs[1], runs[0])
        out["auto"] = dict(best)
        out["auto"]["which_run"] = "run %d of 2 fresh loads (the one with the shorter slowest proof); the other one in other_run" % (1 + runs.index(best))
        out["auto"]["other_run"] = {k: other.get(k) for k in ("cold_ms", "first_proof_ms", "second_proof_ms", "proofs_ms", "first_proof_on_tables", "steady_blocking_ms",
                                                               "time_to_steady_ms", "slowest_proof_after_the_first_over_steady", "converged_pipelined_ms_per_proof")}
        out["always"] = quiet_fresh_key("always")
        # steady state without tables at all (policy never): what a key costs when its 5.6 GiB are not spent
        capi.set_table_policy("never")
        capi.release_tables(pk.handle)
        pipelined(lambda: groth16.prove_begin(pk, inst.w, inst.px, r_, s_), groth16.prove_end, 6, 3)
        samples = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipelined(lambda: groth16.prove_begin(pk, inst.w, inst.px, r_, s_), groth16.prove_end, 10, 3)
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) / 10 * 1e3)
        tm = capi.last_timing()
        p = groth16.prove_resident(pk, inst.w, inst.px, r_, s_)
        out["table_free_steady"] = {"ms_per_proof": statistics.median(samples), "ms_per_proof_reps": samples, "window_bits": tm["window_bits"],
                                    "table_bytes": capi.handle_bytes(pk.handle)[1],
                                    "proof_equals_table_route": (p.PiA, p.PiB, p.PiC) == (ref_proof.PiA, ref_proof.PiB, ref_proof.PiC)}
    finally:
        capi.set_table_policy("always")
        if os.path.exists(path):
            os.remove(path)
    return out


def pipelined(begin, end, count, depth, on_done=None):
    """`count` operations, `depth` in flight; returns what the last end() returned."""
    tickets, last = [], None
    for _ in range(count):
        tickets.append(begin())
        if len(tickets) == depth:
            last = end(tickets.pop(0))
            if on_done:
                on_done()
    while tickets:
        last = end(tickets.pop(0))
        if on_done:
            on_done()
    return last


def _limbs(x):
    """A field element (int < 2^256) -> eight 32-bit limbs, least significant first (float64 holds each exactly); nested tuples of
    them (the coordinates of a point) -> nested lists."""
    if isinstance(x, int):
        return [float((x >> (32 * i)) & 0xFFFFFFFF) for i in range(8)]
    return [_limbs(y) for y in x]


def _point_array(p):
    """A point as the library returns it (None = an MSM at infinity, written as (0, 0)) -> float64 limbs."""
    return np.array(_limbs((0, 0) if p is None else p), dtype=np.float64)


def dump_outputs(out_dir, result):
    """--dump-outputs: what the timed path returned in its last step, one DIR/<name>.npy per array (float64 limbs, see _limbs).
    result: a groth16 / snark Proof, an MSM point, or a list of proofs (one per device; stacked along a leading axis)."""
    os.makedirs(out_dir, exist_ok=True)
    proofs = result if isinstance(result, list) else [result]
    fields = getattr(proofs[0], "FIELDS", ("PiA", "PiB", "PiC")) if hasattr(proofs[0], "PiA") else None
    arrays = ({k: np.stack([_point_array(getattr(p, k)) for p in proofs]) for k in fields} if fields else
              {"msm_g1": np.stack([_point_array(p) for p in proofs])})
    if not isinstance(result, list):
        arrays = {k: v[0] for k, v in arrays.items()}
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    return sorted(arrays)


def live_pmc_traffic(args):
    """HBM traffic of the dominant kernel, measured NOW: bench.py cannot attach counters to itself, so it runs itself twice more under
    rocprofv3 -- one --pmc pass per counter (FETCH_SIZE takes 3 of the 4 TCC slots, WRITE_SIZE 2: they cannot share a pass; no tracing
    domain is combined with --pmc) -- on the same workload with ONE step, and averages the counter over the k_bucket_accumulate<G1>
    dispatches (the 3-array launch over w and the 1-array launch over h: the mix the timed region averages).  Counter unit: KB.
    Returns (dict, None) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if os.environ.get("GS_BENCH_NO_LIVE_PMC") == "1":
        return None, "GS_BENCH_NO_LIVE_PMC=1"
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    res = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="gs_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--pmc", ctr, "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__),
                   "--log2n", str(args.log2n), "--table-policy", args.table_policy, "--steps", "1", "--warmup", "0", "--reps", "1", "--settle-ms", "0",
                   "--cpu-log2n", "0", "--no-extras", "--no-check"]
            env = dict(os.environ, TMPDIR="/tmp", GS_BENCH_NO_LIVE_PMC="1")
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300, check=True)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                return None, "rocprofv3 wrote no counter_collection.csv for %s" % ctr
            vals = []
            with open(files[0]) as f:
                for row in csv.DictReader(f):
                    if row.get("Counter_Name") == ctr and "k_bucket_accumulate<gs::FqTag>" in row.get("Kernel_Name", ""):
                        vals.append(float(row["Counter_Value"]))
            if not vals:
                return None, "no k_bucket_accumulate<G1> dispatch in the %s pass" % ctr
            res[ctr] = (sum(vals) / len(vals) * 1024.0, len(vals))
        except (OSError, subprocess.SubprocessError, ValueError, KeyError) as e:
            return None, "%s pass failed: %s" % (ctr, type(e).__name__)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return {"fetch_bytes_per_launch_raw": res["FETCH_SIZE"][0], "write_bytes_per_launch_raw": res["WRITE_SIZE"][0],
            "dispatches_averaged": [res["FETCH_SIZE"][1], res["WRITE_SIZE"][1]]}, None


def build_stamp():
    """Which library this line was measured with: gs_version() (carries the compile flags) + the source commit recorded by
    __graft_entry__.build() next to the library (the GPU box has no .git)."""
    import hashlib
    stamp = {"library": capi.version()}
    try:
        lib = os.environ.get("GS_LIB") or os.path.join(ROOT, "go-snark-study_amd", "libgosnark_hip.so")
        sha = hashlib.sha256(open(lib, "rb").read()).hexdigest()
        with open(os.path.join(ROOT, "go-snark-study_amd", "BUILD_INFO.json")) as f:
            info = json.load(f)
        if info.get("lib_sha256") == sha:
            stamp["source_commit"] = info.get("commit")
            if info.get("sources_modified_since_commit"):
                stamp["sources_modified_since_commit"] = info["sources_modified_since_commit"]
        else:
            stamp["source_commit"] = "stale: the library was rebuilt after BUILD_INFO.json was written"
    except (OSError, ValueError):
        stamp["source_commit"] = None
    return stamp


def time_calls(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count * 1e3


def time_calls_median(fn, count, reps=3, warm=2):
    """Blocking-call latency the way the pipelined figures are taken: `warm` untimed calls (the blocking slot's workspaces, clocks),
    then the median of `reps` repetitions of `count` calls.  Returns (median, [repetitions])."""
    for _ in range(warm):
        fn()
    samples = [time_calls(fn, count) for _ in range(reps)]
    return statistics.median(samples), samples


def msm_extras(seed):
    """BASELINE metric, second half (G1-MSM terms/s; configs[1] = 2^16 terms): pipelined (three in flight) and blocking."""
    out = {}
    for logn in (20, 16):
        n = 1 << logn
        bases = capi.g1_fixed_base(synth.scalars_u64(n, seed + logn))
        sc = capi.scalars_upload(synth.scalars_u64(n, seed + 77 + logn))
        capi.msm_resident(bases, sc, n)                 # window table + workspaces
        reps = 40 if logn == 20 else 200
        pipelined(lambda: capi.msm_begin(bases, sc, n), capi.msm_end, 12, 3)
        samples = []
        for _ in range(3):                               # median of three timed repetitions (the first one after a size change runs slow)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipelined(lambda: capi.msm_begin(bases, sc, n), capi.msm_end, reps, 3)
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) / reps * 1e3)
        pipe_ms = statistics.median(samples)
        blk_ms = time_calls(lambda: capi.msm_resident(bases, sc, n), reps // 2)
        out["2^%d" % logn] = {"terms_per_s_pipelined": n / pipe_ms * 1e3, "ms_pipelined": pipe_ms, "ms_pipelined_reps": samples,
                              "terms_per_s_blocking": n / blk_ms * 1e3,
                              "ms_blocking": blk_ms, "window_bits": capi.last_timing()["window_bits"]}
        bases.free()
        sc.free()
    return out


def logical_shard_report(args, n, seed, sharded_prove):
    """--logical-shards S on one GPU: S logical devices (gs_init lists GPU 0 S times).  Measures every shard alone, then all shards
    together through gs_groth16_prove_multi / gs_msm_g1_multi with the records passing through ncclAllGather, and MODELS the
    S-GPU time as max(shard) + gather + host tail (the shards would run concurrently on S GPUs)."""
    S = args.logical_shards
    capi.comm_init_local()
    out = {"logical_shards": S}
    if sharded_prove:
        inst = synth.sqchain_setup_instance(n, seed)
        full = inst.device_pk()
        r_, s_ = synth.field_elems(2, seed ^ 0xABCDEF, R)
        want = groth16.prove_resident(full, inst.w, inst.px, r_, s_)
        pks = [groth16.ShardPkTo(full, d, S, d) for d in range(S)]
        full.handle.free()                                  # every logical device keeps 1/S of every key array
        ws = [capi.scalars_clone(inst.w, d) for d in range(S)]
        pxs = [capi.scalars_clone(inst.px, d) for d in range(S)]
        for d in range(S):
            groth16.prove_partials(pks[d], ws[d], pxs[d], d, S)          # window tables of the slice
        shard_ms = [time_calls(lambda d=d: groth16.prove_partials(pks[d], ws[d], pxs[d], d, S), 3) for d in range(S)]
        poly_ms = capi.device_timing(0)["poly_ms"]

        def step():
            return groth16.prove_multi(pks, ws, pxs, r_, s_)[0]
        got, used = groth16.prove_multi(pks, ws, pxs, r_, s_)
        if (got.PiA, got.PiB, got.PiC) != (want.PiA, want.PiB, want.PiC):
            raise SystemExit("bench.py: the sharded proof differs from the single-device proof")
        ok = groth16.VerifyProof(inst.vk, got, capi.u64_to_ints(inst.w_host[1:2]))
        out.update({"proof_equals_single_device": True, "proof_verified": bool(ok), "used_rccl": used,
                    "replicated_poly_stage_ms": poly_ms})
        if sum(capi.pk_eval_count(k.handle) for k in pks) == n:
            # The values route (gs_groth16_witness_values on ONE owner per proof, slices of H's values scattered, every shard sums only
            # its term ranges): no replicated polynomial stage.  Measured here: the owner's stage, every shard alone, the proof itself.
            from gosnark_amd import r1csqap
            capi.set_device(0)
            dr = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
            hv, bad = groth16.witness_values(pks[0], dr, ws[0])
            assert bad == 0
            values_ms = time_calls(lambda: groth16.witness_values(pks[0], dr, ws[0], hv), 4)
            slices = groth16.scatter_values(hv, S)

            def scatter_once():
                for h in groth16.scatter_values(hv, S):
                    h.free()
            scatter_ms = time_calls(scatter_once, 3)
            for d in range(S):
                groth16.prove_partials_values(pks[d], ws[d], slices[d], d, S)       # evaluation-basis tables of the slice
            v_ms = [time_calls(lambda d=d: groth16.prove_partials_values(pks[d], ws[d], slices[d], d, S), 3) for d in range(S)]
            # ... and streamed: three shard operations of one device in flight (what a rank does with consecutive proofs)
            def stream(d, count):
                pipelined(lambda: groth16.partials_values_begin(pks[d], ws[d], slices[d], d, S), groth16.partials_end, count, 3)
            vp_ms = []
            for d in (0, S - 1):
                stream(d, 6)                                   # the device's three ticket slots allocate their workspaces on first use
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stream(d, 12)
                torch.cuda.synchronize()
                vp_ms.append((time.perf_counter() - t0) / 12 * 1e3)
            gotv, usedv = groth16.prove_multi_values(pks, ws, slices, r_, s_)
            if (gotv.PiA, gotv.PiB, gotv.PiC) != (want.PiA, want.PiB, want.PiC):
                raise SystemExit("bench.py: the values-route sharded proof differs from the single-device proof")
            out["values_route"] = {"owner_polynomial_stage_ms": values_ms, "per_shard_ms": v_ms, "per_shard_ms_three_in_flight": vp_ms, "proof_equals_single_device": True,
                                   "scatter_payload_bytes_per_peer": 32 * (n // S), "scatter_on_one_gpu_ms": scatter_ms, "used_rccl": usedv}
        unit = "constraints/s"
    else:
        from gosnark_amd import parallel
        bases = capi.g1_fixed_base(synth.scalars_u64(n, seed))
        sc = capi.scalars_upload(synth.scalars_u64(n, seed + 77))
        want = capi.msm_resident(bases, sc, n)
        bs, ss = [], []
        for d in range(S):
            lo, hi = parallel.shard_range(n, S, d)
            bs.append(capi.g1_clone(bases, d, lo, hi - lo))
            ss.append(capi.scalars_clone(sc, d, lo, hi - lo))
        bases.free()
        for d in range(S):
            capi.msm_resident(bs[d], ss[d], len(ss[d]))
        shard_ms = [time_calls(lambda d=d: capi.msm_resident(bs[d], ss[d], len(ss[d])), 5) for d in range(S)]

        def step():
            return capi.msm_multi(bs, ss)[0]
        got, used = capi.msm_multi(bs, ss)
        if got != want:
            raise SystemExit("bench.py: the sharded MSM differs from the single-device MSM")
        out.update({"result_equals_single_device": True, "used_rccl": used})
        unit = "terms/s"
    # the exchange alone: S records through ncclAllGather (1 rank here: the latency floor of the collective, not xGMI)
    blob = bytes(416 * S)
    gather_ms = time_calls(lambda: capi.comm_allgather(blob, 1), 50)
    out["per_shard_ms"] = shard_ms
    out["gather_ms_one_rank_rccl"] = gather_ms
    out["collectives_so_far"] = capi.comm_info()["collectives"]
    return step, out, unit


STRONG_MSM_GOLDEN = os.path.join(ROOT, "tests", "golden", "oracle_msm_g1_2p22.json")     # configs[3]: 2^22 terms, expected point from the naive loops


def device_report(devs):
    """Which GPUs the N devices of this job are, and whether they reach each other (hipDeviceCanAccessPeer, asked through torch)."""
    phys = sorted(set(int(d) for d in devs))
    rep = {"logical_to_physical": [int(d) for d in devs], "visible_gpus": torch.cuda.device_count(),
           "names": [torch.cuda.get_device_name(d) for d in phys]}
    try:
        rep["can_access_peer"] = [[1 if a == b else int(torch.cuda.can_device_access_peer(a, b)) for b in phys] for a in phys]
    except Exception as e:          # noqa: BLE001 -- a report, never a reason to lose the line
        rep["can_access_peer"] = "unavailable: %s" % type(e).__name__
    return rep


class LineGuard:
    """The first real multi-GPU run must not lose its line to a section nobody could execute before it (a collective one rank never
    enters hangs the others for good).  Rank 0 parks the line it has so far here; a guarded section that overruns its budget makes
    rank 0 print that line with the reason, and every rank leaves the process."""

    def __init__(self, rank):
        self.rank, self.line, self.timer, self.section = rank, None, None, None

    def arm(self, seconds, section):
        import threading
        self.disarm()
        self.section = section

        def fire():
            if self.rank == 0 and self.line is not None:
                try:
                    out = dict(self.line)
                    out["strong"] = dict(out.get("strong") or {}, watchdog="section '%s' did not finish within %d s: the line was printed without it" % (self.section, seconds))
                    print(json.dumps(out), flush=True)
                except Exception:       # noqa: BLE001
                    pass
            os._exit(0)
        self.timer = threading.Timer(seconds + (0 if self.rank == 0 else 5), fire)
        self.timer.daemon = True
        self.timer.start()

    def disarm(self):
        if self.timer is not None:
            self.timer.cancel()
            self.timer = None


def _err(e):
    return {"error": "%s: %s" % (type(e).__name__, str(e)[:400])}


def _same_proof(p, q):
    return (p.PiA, p.PiB, p.PiC) == (q.PiA, q.PiB, q.PiC)


def _golden_msm():
    with open(STRONG_MSM_GOLDEN) as f:
        rec = json.load(f)
    return rec["n"], rec["seed_bases"], rec["seed_scalars"], (int(rec["x"]), int(rec["y"]))


def strong_one_process(args, ndev, inst, r_, s_, guard):
    """BASELINE configs[3] in ONE process over the `ndev` devices of gs_init (strong scaling; groth16.go:243-250,269-271: the terms of
    every sum are independent): ONE 2^log2n proof through gs_groth16_prove_multi (every device computes H(x)) and through
    gs_groth16_prove_multi_values (the owner's polynomial stage once, H's values scattered with gs_scalars_clone = hipMemcpyPeerAsync
    between different GPUs), and ONE 2^22-term G1 MSM through gs_msm_g1_multi.  The 416-byte / 72-byte records pass through
    ncclAllGather when gs_comm_init_local made a communicator (`used_rccl`).  Every figure is a blocking call per step."""
    from gosnark_amd import parallel, r1csqap
    n, K = inst.n, max(3, min(args.steps, 5))
    strong = {"mode": "one process, %d devices (gs_groth16_prove_multi / gs_groth16_prove_multi_values / gs_msm_g1_multi)" % ndev, "steps": K}
    if guard.line is not None:
        guard.line["strong"] = strong
    key = "prove_sharded_2^%d" % args.log2n
    pk0 = inst.device_pk()
    pks = ws = pxs = None
    guard.arm(args.strong_budget_s, key)
    try:
        capi.set_device(0)
        want = groth16.prove_resident(pk0, inst.w, inst.px, r_, s_)
        single_ms = time_calls(lambda: groth16.prove_resident(pk0, inst.w, inst.px, r_, s_), K)
        pks = [groth16.ShardPkTo(pk0, d, ndev, d) for d in range(ndev)]          # device d keeps slice d of every key array
        ws = [capi.scalars_clone(inst.w, d) for d in range(ndev)]
        pxs = [capi.scalars_clone(inst.px, d) for d in range(ndev)]
        got, used = groth16.prove_multi(pks, ws, pxs, r_, s_)                    # (window tables of the slices)
        ms = time_calls(lambda: groth16.prove_multi(pks, ws, pxs, r_, s_), K)
        strong[key] = {"px_route": {"ms_per_step": ms, "value": n / ms * 1e3, "unit": "constraints/s", "proof_equals_single_device": _same_proof(got, want),
                                    "used_rccl": used, "replicated_polynomial_stage_ms": capi.device_timing(0)["poly_ms"]},
                       "single_device_blocking_ms": single_ms}
    except Exception as e:          # noqa: BLE001
        strong[key] = _err(e)
    if pks is not None and "error" not in strong[key]:
        try:
            if sum(capi.pk_eval_count(k.handle) for k in pks) != n:
                raise RuntimeError("the key slices carry no evaluation-basis array")
            drs = []
            for d in range(ndev):
                capi.set_device(d)
                drs.append(r1csqap.DeviceR1CS(*inst.r1cs, inst.m))
            hv = [None] * ndev
            state = {"i": 0, "owner_ms": 0.0, "scatter_ms": 0.0}

            def one():
                o = state["i"] % ndev                                    # the devices take turns as owner of a proof's polynomial stage
                state["i"] += 1
                t0 = time.perf_counter()
                capi.set_device(o)
                hv[o], bad = groth16.witness_values(pks[o], drs[o], ws[o], hv[o])
                if bad:
                    raise RuntimeError("the benchmark witness violates a constraint")
                t1 = time.perf_counter()
                slices = []
                for d in range(ndev):
                    lo, hi = parallel.shard_range(n, ndev, d)
                    slices.append(capi.scalars_clone(hv[o], d, lo, hi - lo))
                t2 = time.perf_counter()
                res = groth16.prove_multi_values(pks, ws, slices, r_, s_)
                for h in slices:
                    h.free()
                state["owner_ms"] += (t1 - t0) * 1e3
                state["scatter_ms"] += (t2 - t1) * 1e3
                return res
            for _ in range(ndev):                                        # every owner once: its workspaces, the slices' evaluation-basis tables
                gotv, usedv = one()
            state.update(owner_ms=0.0, scatter_ms=0.0)
            ms = time_calls(one, K)
            capi.set_device(0)
            strong[key]["values_route"] = {"ms_per_step": ms, "value": n / ms * 1e3, "unit": "constraints/s", "proof_equals_single_device": _same_proof(gotv, want),
                                           "used_rccl": usedv, "owner_polynomial_stage_ms": state["owner_ms"] / K, "scatter_ms": state["scatter_ms"] / K,
                                           "scatter_payload_bytes_per_peer": 32 * (n // ndev), "owner": "rotates: proof i on device i mod N"}
            for h in hv + [d_.handle for d_ in drs]:
                if h is not None:
                    h.free()
        except Exception as e:      # noqa: BLE001
            strong[key]["values_route"] = _err(e)
    for h in (ws or []) + (pxs or []) + [k.handle for k in (pks or [])]:
        h.free()
    # --- configs[3]: one 2^22-term G1 MSM over the N devices, expected point = the naive-loop golden of tests/golden ---
    guard.arm(args.strong_budget_s, "msm_sharded_2^22")
    try:
        n22, sb, ssd, want_pt = _golden_msm()
        capi.set_device(0)
        bases = capi.g1_fixed_base(synth.scalars_u64(n22, sb))
        sc = capi.scalars_upload(synth.scalars_u64(n22, ssd))
        got1 = capi.msm_resident(bases, sc, n22)
        single_ms = time_calls(lambda: capi.msm_resident(bases, sc, n22), K)
        capi.release_tables(bases)
        bs, ss = [], []
        for d in range(ndev):
            lo, hi = parallel.shard_range(n22, ndev, d)
            bs.append(capi.g1_clone(bases, d, lo, hi - lo))
            ss.append(capi.scalars_clone(sc, d, lo, hi - lo))
        bases.free()
        sc.free()
        got, used = capi.msm_multi(bs, ss)
        ms = time_calls(lambda: capi.msm_multi(bs, ss), K)
        strong["msm_sharded_2^22"] = {"ms_per_step": ms, "value": n22 / ms * 1e3, "unit": "terms/s", "terms": n22,
                                      "equals_naive_loop_golden": bool(got == want_pt and got1 == want_pt), "used_rccl": used, "single_device_blocking_ms": single_ms}
        for h in bs + ss:
            h.free()
    except Exception as e:          # noqa: BLE001
        strong["msm_sharded_2^22"] = _err(e)
    try:
        if capi.comm_info()["nranks"] > 0:
            blob = bytes(416 * capi.comm_info()["nranks"])
            strong["gather_ms"] = time_calls(lambda: capi.comm_allgather(blob, capi.comm_info()["nranks"], capi.comm_info()["nranks"]), 20)
    except Exception as e:          # noqa: BLE001
        strong["gather_ms"] = _err(e)
    guard.disarm()
    return strong

def strong_ranks(args, world, rank, share, inst, pk_full, r_, s_, guard, cpu_collectives=None):
    """BASELINE configs[3] with one process per GPU (strong scaling; every rank holds the same instance): ONE 2^log2n proof through
    gs_groth16_prove_sharded (every rank computes H(x)) and through the values route (owner = proof index mod N runs
    gs_groth16_witness_values, gs_scalars_scatter = one ncclSend/ncclRecv group, gs_groth16_prove_sharded_values), and ONE 2^22-term G1
    MSM through gs_msm_g1_sharded; the partial points are gathered INSIDE the library over the communicator of gs_comm_init_rank
    (ncclCommInitRank, unique id carried by torch.distributed).  GS_BENCH_SHARE_GPU=1 (all ranks on one GPU, gloo) takes the
    torch.distributed twins of the exchanges instead (RCCL refuses two ranks on one device).  Every rank runs this; rank 0 reports."""
    from gosnark_amd import parallel, r1csqap
    n, K = inst.n, max(3, min(args.steps, 5))
    tdev = "cpu" if (share if cpu_collectives is None else cpu_collectives) else "cuda"
    strong = {"mode": "one process per GPU, %d ranks" % world, "steps": K}
    if guard.line is not None:
        guard.line["strong"] = strong

    def agree(ok):
        t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=tdev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item() == 1.0)

    def timed(fn, count):
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        dist.barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=tdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) / count * 1e3

    use_rccl, comm_err = not share, None
    if use_rccl:
        guard.arm(args.strong_budget_s, "gs_comm_init_rank (ncclCommInitRank)")
        ok = True
        try:
            uid = [capi.comm_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            capi.comm_init_rank(uid[0], world, rank)
        except Exception as e:          # noqa: BLE001
            ok, comm_err = False, str(e)[:300]
        if not agree(ok):
            capi.comm_destroy()
            use_rccl = False
            comm_err = comm_err or "another rank could not join the communicator"
    strong["exchange"] = ("in-library RCCL (ncclAllGather of byte records, ncclSend/ncclRecv scatter)" if use_rccl else
                          "torch.distributed %s twins of the exchanges (parallel.allgather_points / scatter_scalars)" % dist.get_backend())
    if comm_err:
        strong["communicator_error"] = comm_err
    key = "prove_sharded_2^%d" % args.log2n
    pk = None
    guard.arm(args.strong_budget_s, key)
    try:
        want = groth16.prove_resident(pk_full, inst.w, inst.px, r_, s_)
        single_ms = time_calls(lambda: groth16.prove_resident(pk_full, inst.w, inst.px, r_, s_), K)
        pk = groth16.ShardPk(pk_full, rank, world)            # this rank's 1/N slice of every key array (window tables for the slice only)

        def pstep():
            return (groth16.prove_sharded_rccl(pk, inst.w, inst.px, r_, s_) if use_rccl else groth16.prove_sharded(pk, inst.w, inst.px, r_, s_))
        got = pstep()
        ms = timed(pstep, K)
        strong[key] = {"px_route": {"ms_per_step": ms, "value": n / ms * 1e3, "unit": "constraints/s", "proof_equals_single_device": agree(_same_proof(got, want)),
                                    "replicated_polynomial_stage_ms": capi.last_timing()["poly_ms"]},
                       "single_device_blocking_ms": single_ms}
    except Exception as e:              # noqa: BLE001 -- (a rank that fails alone leaves the others in a collective: the guard ends that)
        strong[key] = _err(e)
    if pk is not None and "error" not in strong[key]:
        guard.arm(args.strong_budget_s, key + " values route")
        try:
            if not capi.pk_eval_count(pk.handle):
                raise RuntimeError("the key slice carries no evaluation-basis array")
            dr = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
            st = {"i": 0, "hv": None, "mine": None}

            def vstep():
                owner = parallel.owner_of(st["i"], world)
                st["i"] += 1
                if rank == owner:
                    st["hv"], bad = groth16.witness_values(pk, dr, inst.w, st["hv"])
                    if bad:
                        raise RuntimeError("the benchmark witness violates a constraint")
                if use_rccl:
                    st["mine"] = capi.scalars_scatter(st["hv"] if rank == owner else None, n, owner, st["mine"])
                    return groth16.prove_sharded_values_rccl(pk, inst.w, st["mine"], r_, s_)
                sl = parallel.scatter_scalars(capi.scalars_download(st["hv"]) if rank == owner else None, n, owner)
                mine = capi.scalars_upload(sl)
                pts, flags = groth16.prove_partials_values(pk, inst.w, mine, rank, world)
                mine.free()
                return groth16.finish(pk, parallel.combine_partials(parallel.allgather_points(pts, flags), flags), r_, s_)
            for _ in range(world):
                gotv = vstep()
            ms = timed(vstep, K)
            strong[key]["values_route"] = {"ms_per_step": ms, "value": n / ms * 1e3, "unit": "constraints/s", "proof_equals_single_device": agree(_same_proof(gotv, want)),
                                           "scatter_payload_bytes_per_peer": 32 * (n // world), "owner": "rotates: proof i on rank i mod N"}
            if use_rccl and st["hv"] is None:
                st["hv"], _ = groth16.witness_values(pk, dr, inst.w, None)
            if use_rccl:
                own = timed(lambda: groth16.witness_values(pk, dr, inst.w, st["hv"]), K)       # every rank at once: the owner's stage alone
                sc_ms = timed(lambda: capi.scalars_scatter(st["hv"] if rank == 0 else None, n, 0, st["mine"]), K)
                strong[key]["values_route"].update(owner_polynomial_stage_ms=own, scatter_ms=sc_ms)
        except Exception as e:          # noqa: BLE001
            strong[key]["values_route"] = _err(e)
    guard.arm(args.strong_budget_s, "msm_sharded_2^22")
    try:
        n22, sb, ssd, want_pt = _golden_msm()
        lo, hi = parallel.shard_range(n22, world, rank)
        bases = capi.g1_fixed_base(np.ascontiguousarray(synth.scalars_u64(n22, sb)[lo:hi]))
        sc = capi.scalars_upload(np.ascontiguousarray(synth.scalars_u64(n22, ssd)[lo:hi]))

        def mstep():
            return capi.msm_sharded(bases, sc) if use_rccl else parallel.msm_g1_sharded(bases, sc, hi - lo)
        got = mstep()
        ms = timed(mstep, K)
        strong["msm_sharded_2^22"] = {"ms_per_step": ms, "value": n22 / ms * 1e3, "unit": "terms/s", "terms": n22,
                                      "equals_naive_loop_golden": agree(got == want_pt)}
        bases.free()
        sc.free()
    except Exception as e:              # noqa: BLE001
        strong["msm_sharded_2^22"] = _err(e)
    if use_rccl:
        try:
            blob = bytes(416)
            strong["gather_ms"] = timed(lambda: capi.comm_allgather(blob, world), 20)
        except Exception as e:          # noqa: BLE001
            strong["gather_ms"] = _err(e)
    guard.disarm()
    return strong

def rccl_report(mode, err=None):
    try:
        info = capi.comm_info()
    except Exception as e:          # noqa: BLE001
        return {"mode": mode, "error": str(e)[:200]}
    rep = {"mode": mode, "ranks_seen": info["nranks"], "local": info["local"], "collectives": info["collectives"]}
    if err:
        rep["error"] = err
    return rep


def base_line(args, n, world, value, elapsed, rep_elapsed, workload, parallelism, instance, scaling="weak"):
    return {
        "metric": "Groth16 constraints/sec (prove) at 2^%d R1CS" % args.log2n,
        "value": value, "unit": "constraints/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "reps": len(rep_elapsed), "ms_per_step_reps": [e / args.steps * 1e3 for e in rep_elapsed],
        "ms_per_step_min": min(rep_elapsed) / args.steps * 1e3,
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": "u32 (9x29-bit Montgomery limbs of the 254-bit BN128 fields)", "data": "synthetic",
        "config": {"workload": workload, "settle_ms_before_warmup": args.settle_ms, "proofs_in_flight": 3, "constraints": n, "variables": n + 1, "npublic": 1,
                   "parallelism": parallelism, "instance": instance},
    }


def accumulate_roofline(tm, launches_key="acc_g1_launches"):
    """`roofline` / `roofline_valu` of the dominant kernel from one gs_timing record (HIP events on the library's stream)."""
    launches = max(tm[launches_key], 1)
    avg_s = tm["acc_g1_ms"] / launches * 1e-3
    bpl = G1_TERM_BYTES * tm["acc_g1_terms"] / launches
    ach = bpl / avg_s / 1e9 if avg_s > 0 else 0.0
    mads = tm["acc_g1_adds"] / launches * MADS_PER_MIXED_ADD / avg_s / 1e12 if avg_s > 0 else 0.0
    return ({"bound": "hbm", "kernel": "k_bucket_accumulate<G1>", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
             "traffic": None, "avg_launch_ms": avg_s * 1e3, "algorithmic_bytes_per_launch": bpl,
             "note": "integer-issue bound (254-bit modular arithmetic on 32-bit VALU), see DESIGN.md section 5; traffic is measured by the single-GPU run"},
            {"bound": "valu-int-mad", "kernel": "k_bucket_accumulate<G1>", "achieved": mads, "peak": MAD_PEAK_T, "unit": "T lane-mad/s", "frac": mads / MAD_PEAK_T})


def main_one_process(args):
    """`python bench.py --gpus N` without a launcher: this process drives the N devices (see the module docstring)."""
    from gosnark_amd import r1csqap
    N = args.gpus
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: there is no CPU path for the product code")
    visible = torch.cuda.device_count()
    devs = [d % visible for d in range(N)]
    capi.init(devs)
    capi.set_table_policy(args.table_policy)       # steady state on window tables (built inside the untimed warm-up), as main()
    if args.window_bits or os.environ.get("GS_BENCH_C"):
        capi.set_window_bits(args.window_bits or int(os.environ["GS_BENCH_C"]))
    guard = LineGuard(0)
    n = 1 << args.log2n
    seed = 0x5EED0002
    r_, s_ = synth.field_elems(2, seed ^ 0xABCDEF, R)

    # --- weak scaling (BASELINE configs[4]): the same circuit and key on every device, every device its own witness / public input ---
    capi.set_device(0)
    inst = synth.sqchain_setup_instance(n, seed)
    pk0 = inst.device_pk()
    pks, replica_note = [pk0], "GPU-to-GPU copies of device 0's key (gs_groth16_pk_shard_to)"
    for d in range(1, N):
        try:
            pks.append(groth16.ShardPkTo(pk0, 0, 1, d))                           # a full replica, copied GPU to GPU
        except Exception as e:          # noqa: BLE001 -- peer copies have never met a second physical GPU: build the same key in place
            capi.set_device(d)
            pks.append(synth.sqchain_setup_instance(n, seed).device_pk())
            capi.set_device(0)
            replica_note = "peer copy failed (%s): the same deterministic setup was run on the device instead" % str(e)[:120]
    xs = [capi.u64_to_ints(inst.w_host[1:2])[0]] + synth.field_elems(N - 1, seed + 4242)
    ws, pxs = [inst.w], [inst.px]
    for d in range(1, N):
        capi.set_device(d)
        dr = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
        ws.append(capi.scalars_upload(synth.sqchain_witness(n, xs[d])))
        pxs.append(dr.ComputePxResident(ws[d]))
        dr.handle.free()
    capi.set_device(0)
    rs = [tuple(synth.field_elems(2, seed + 99 + d, R)) for d in range(N)]

    def batch(steps):
        """`steps` steps = steps x N proofs, proof i on device i mod N, three in flight per device (gs_groth16_prove_batch)"""
        idx = [i % N for i in range(steps * N)]
        return groth16.prove_batch(pks, [ws[d] for d in idx], [pxs[d] for d in idx], [rs[d] for d in idx])

    def sync_all():
        for d in sorted(set(devs)):
            torch.cuda.synchronize(d)
    batch(3)                                                   # window tables, the three ticket slots' workspaces
    t_settle = time.perf_counter()
    while args.settle_ms > 0 and (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
        batch(max(1, min(args.steps, 4)))
    if args.warmup > 0:
        batch(args.warmup)
    rep_elapsed, last = [], None
    for _ in range(max(1, args.reps)):
        sync_all()
        t0 = time.perf_counter()
        last = batch(args.steps)
        sync_all()
        rep_elapsed.append(time.perf_counter() - t0)
    elapsed = statistics.median(rep_elapsed)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last[-N:])             # the last step: one proof per device
    if args.full:
        good = all(groth16.VerifyProof(inst.vk, last[-N + d], [xs[d]]) and not groth16.VerifyProof(inst.vk, last[-N + d], [xs[(d + 1) % N] if N > 1 else (xs[d] + 1) % R])
                   for d in range(N))
        if not good:
            raise SystemExit("bench.py: groth16.VerifyProof rejected a device's proof (or accepted it for another device's public input)")
    spread = ("%d GPUs" % N) if visible >= N else ("%d LOGICAL devices on %d visible GPU(s): NOT a multi-GPU measurement" % (N, visible))
    out = base_line(args, n, N, n * N * args.steps / elapsed, elapsed, rep_elapsed,
                    "groth16_prove_2^%d_constraints_per_gpu" % args.log2n,
                    "independent proofs, one stream of proofs per GPU, one process drives %s (gs_groth16_prove_batch, three in flight per device, no collective)" % spread,
                    inst.describe() + "; the same key on every device, a different witness / public input per device")
    tm = capi.device_timing(0)
    out["config"]["window_bits"] = tm["window_bits"]
    out["roofline"], out["roofline_valu"] = accumulate_roofline(tm)
    if args.full:
        out["proof_verified"] = "groth16.VerifyProof accepted each device's last proof for its own public input and rejected it for another's (%d/%d devices)" % (N, N)
    out["launch"] = "one process, no launcher (WORLD_SIZE unset)"
    out["config"]["key_replicas"] = replica_note
    out["devices"] = device_report(devs)
    out["build"] = build_stamp()
    guard.line = out
    for d in range(1, N):
        for h in (ws[d], pxs[d], pks[d].handle):
            h.free()
    if args.full:
        # The communicator is created only now: the weak-scaling workload above needs none (independent proofs, no collective), and with the
        # line already parked in the guard a first ncclCommInitAll that never returns costs the strong section, not the measurement.
        comm_err = None
        guard.arm(args.strong_budget_s, "gs_comm_init_local (ncclCommInitAll)")
        try:
            capi.comm_init_local()           # one RCCL rank per distinct physical device; the records of the sharded workloads travel through it
        except Exception as e:              # noqa: BLE001 -- the sharded workloads fall back to host memory
            comm_err = str(e)[:300]
        guard.disarm()
        if not args.no_strong:
            out["strong"] = strong_one_process(args, N, inst, r_, s_, guard)
        out["rccl"] = rccl_report("local: ncclCommInitAll over the distinct physical devices of this process (gs_comm_init_local)", comm_err)
        guard.disarm()
    import ctypes
    ctypes.CDLL(None).fflush(None)
    print(json.dumps(out), flush=True)

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settle-ms", type=float, default=400.0, help="untimed steps before the W warm-up steps until this many ms have passed (0 = none)")
    ap.add_argument("--reps", type=int, default=None, help="repetitions of the timed K steps; the median repetition is reported "
                                                            "(default: 1, or 5 with --full)")
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--workload", default="prove", choices=["prove", "prove_from_r1cs", "prove_witness", "prove_sharded", "prove_pinocchio", "msm_g1", "msm_sharded"],
                    help="prove: one independent proof per GPU (weak scaling, the default the driver runs); prove_sharded: ONE proof "
                         "whose MSM term ranges are split over the ranks (strong scaling, in-library RCCL gather of 416-byte records); "
                         "prove_from_r1cs: every step also rebuilds px from the resident sparse R1CS and witness -- the "
                         "stage upstream of GenerateProofs, reported for information; prove_witness: witness -> proof without px "
                         "(gs_groth16_prove_witness[_begin]: BASELINE configs[2] as worded, 'full prove + QAP kernels'), the h-MSM over H's values "
                         "when the key carries the evaluation-basis PowersTauDelta")
    ap.add_argument("--sharded-route", default="px", choices=["px", "values"],
                    help="prove_sharded with one process per GPU: px = every rank computes H(x) itself (replicated polynomial stage); values = "
                         "the ranks take turns as owner of a proof's polynomial stage (gs_groth16_witness_values), the owner scatters H's values "
                         "(gs_scalars_scatter) and every rank sums only its term ranges (gs_groth16_prove_sharded_values)")
    ap.add_argument("--logical-shards", type=int, default=0,
                    help="prove_sharded / msm_sharded on ONE GPU: that many logical devices in this process (configs[3] stand-in, SURVEY 8e)")
    ap.add_argument("--instance", default="setup", choices=["setup", "realistic", "gates", "sqchain", "random"],
                    help="setup: sqchain R1CS + structured trusted setup on the device + px from the sparse system (a complete, "
                         "checkable instance, SURVEY 8d); realistic: the same machinery on an R1CS whose witness has the shape the reference's "
                         "CalculateWitness produces (circuit.go:158-182: about half zeros and ones, most of the rest below 2^32, few full-width "
                         "values); gates: flattened `*` / `+` gates in the shape of the reference's circuit compiler (circuit.go:84-139): two thirds of "
                         "the key's B points are infinity, full-width witness; sqchain: same R1CS with key points k_i*G; random: uniform w / px")
    ap.add_argument("--pipeline", type=int, default=3, choices=[1, 2, 3, 4],
                    help="operations in flight per GPU (prove / msm_g1 workloads): >= 2 = gs_groth16_prove_begin/_end (gs_msm_g1_begin/"
                         "gs_msm_end), the next operation's plan and accumulations are queued behind the current one's; 1 = one "
                         "blocking call per step")
    ap.add_argument("--no-check", action="store_true", help="skip the closed-form proof check of the `setup` instance")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra measurements of the default single-GPU run")
    ap.add_argument("--cpu-log2n", type=int, default=13, help="constraints of the CPU-baseline sample (0 = skip every CPU baseline)")
    ap.add_argument("--table-policy", default="always", choices=["auto", "always", "never"],
                    help="gs_set_table_policy for the timed workload (always: window tables, the steady state of rounds 1-4; never: table-free)")
    ap.add_argument("--window-bits", type=int, default=0, help="force the Pippenger window width (0 = the library's choice)")
    ap.add_argument("--multi", default="one-process", choices=["one-process", "ranks"],
                    help="--gpus N > 1 WITHOUT a launcher (WORLD_SIZE unset): one-process = this process drives the N devices through the library's "
                         "multi-device entry points; ranks = re-execute this command line under torch.distributed.run (one rank per GPU)")
    ap.add_argument("--no-strong", action="store_true", help="N > 1: skip the strong-scaling figures (`strong`) of the line")
    ap.add_argument("--strong-budget-s", type=int, default=240, help="N > 1: a strong-scaling section that runs longer than this is abandoned "
                                                                      "and the line is printed without it")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: proof checks, the extra single-GPU measurements (other routes, the cold path, "
                         "MSM figures, live PMC traffic), CPU baselines, the reference's wasm prover, strong scaling for N > 1, 5 repetitions")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (field elements as eight "
                         "32-bit limbs in float64, least significant first)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 5 if args.full else 1

    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        if args.multi == "ranks":
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
                   "--master-port", str(29500 + os.getpid() % 400), os.path.abspath(__file__)] + sys.argv[1:]
            raise SystemExit(subprocess.call(cmd))       # the same command line under the launcher, in a child process
        if args.workload == "prove" and not args.logical_shards:
            return main_one_process(args)
        raise SystemExit("bench.py --gpus %d --workload %s needs a launcher (python -m torch.distributed.run --nproc-per-node %d bench.py ...) or --multi ranks; "
                         "the default workload runs plainly" % (args.gpus, args.workload, args.gpus))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: there is no CPU path for the product code")
    # development aid for 1-GPU boxes: GS_BENCH_SHARE_GPU=1 maps every rank to device 0 and uses gloo, so the multi-process
    # code path (barriers, max-over-ranks timing, the partial-point gather) can be exercised without a second GPU
    share = os.environ.get("GS_BENCH_SHARE_GPU") == "1"
    launch_notes = []
    if not share and world > torch.cuda.device_count():
        # more ranks than visible GPUs: the ranks share what there is (RCCL refuses two ranks on one device -> gloo for the barriers)
        share = True
        launch_notes.append("%d ranks on %d visible GPU(s): ranks share devices, gloo collectives" % (world, torch.cuda.device_count()))
    if share:
        local = local % max(torch.cuda.device_count(), 1) if os.environ.get("GS_BENCH_SHARE_GPU") != "1" else 0
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # Control plane (barriers, max-over-ranks of a few words, the communicator's unique id) on gloo, ALWAYS: the weak-scaling
        # workload has no data-path collective, so nothing before its line is parked in the watchdog may depend on a library that has
        # never met these GPUs.  RCCL carries the data plane -- the strong section's in-library communicator (ncclCommInitRank,
        # ncclAllGather, ncclSend/ncclRecv) and a torch nccl-group probe -- each behind the watchdog, after the line exists.
        cpu_collectives = True
        dist.init_process_group("gloo")
        launch_notes.append("control plane (barriers, max over ranks) on gloo; RCCL: the in-library communicator of the strong section and a torch nccl-group all_reduce probe")
    if world == 1:
        cpu_collectives = False
    guard = LineGuard(rank)
    logical = args.logical_shards if (args.logical_shards > 1 and world == 1 and args.workload in ("prove_sharded", "msm_sharded")) else 0
    capi.init([local] * logical if logical else local)
    # Steady state = a key whose window tables exist (gs_set_table_policy `always`: built inside the first, untimed, warm-up proof, as
    # in rounds 1-4).  The library's default is `auto`; the cold path and the table-free steady state are measured in the extras.
    capi.set_table_policy(args.table_policy)
    if args.window_bits or os.environ.get("GS_BENCH_C"):
        capi.set_window_bits(args.window_bits or int(os.environ["GS_BENCH_C"]))

    n = 1 << args.log2n
    one_job = args.workload in ("prove_sharded", "msm_sharded")           # ONE proof / MSM for the whole job: strong scaling
    seed = 0x5EED0002 + (0 if one_job else rank)
    sharded = args.workload == "prove_sharded"
    from_r1cs = args.workload == "prove_from_r1cs"
    from_witness = args.workload == "prove_witness"
    shard_info, unit_override = None, None
    rccl_sharded = one_job and world > 1 and not share
    if rccl_sharded:
        # one process per GPU: rank 0's unique id travels over torch.distributed, the gather itself runs inside the library
        uid = [capi.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        capi.comm_init_rank(uid[0], world, rank)
    inst = None
    if logical:
        step, shard_info, unit_override = logical_shard_report(args, n, seed, sharded)
        units_per_step = n
        workload = ("groth16_prove_2^%d_constraints_over_%d_logical_devices_of_one_gpu" if sharded else
                    "g1_msm_2^%d_terms_over_%d_logical_devices_of_one_gpu") % (args.log2n, logical)
    elif sharded or from_r1cs or from_witness or args.workload == "prove":
        args.workload = "prove"
        # N ranks, default instance: the SAME circuit and key on every rank (the setup is deterministic in its seed) and a different
        # witness / public input per rank -- configs[4]'s batch of independent proofs of one circuit; it also gives the strong-scaling
        # sections below one instance every rank holds.
        key_seed = 0x5EED0002 if args.instance == "setup" else seed
        inst = (synth.sqchain_setup_instance(n, key_seed) if args.instance == "setup" else
                synth.realistic_setup_instance(n, seed) if args.instance == "realistic" else
                synth.gates_setup_instance(n, seed) if args.instance == "gates" else
                synth.sqchain_instance(n, seed) if args.instance == "sqchain" else synth.random_instance(n, seed))
        pk = inst.device_pk()
        w_dev, px_dev = inst.w, inst.px
        x_pub = capi.u64_to_ints(inst.w_host[1:2])[0] if args.instance in ("setup", "realistic", "gates") else None
        if args.instance == "setup" and rank > 0 and not one_job:
            from gosnark_amd import r1csqap as _rq
            x_pub = synth.field_elems(1, key_seed + 4242 + rank)[0]
            _dr = _rq.DeviceR1CS(*inst.r1cs, inst.m)
            w_dev = capi.scalars_upload(synth.sqchain_witness(n, x_pub))
            px_dev = _dr.ComputePxResident(w_dev)
            _dr.handle.free()
        if sharded and world > 1:
            # each GPU keeps only its 1/world slice of every proving-key array (and builds window tables for that
            # slice only); the full key this rank built for the setup is released
            full = pk
            pk = groth16.ShardPk(full, rank, world)
            full.handle.free()
        r_, s_ = synth.field_elems(2, seed ^ 0xABCDEF, R)

        dev_r1cs = None
        if from_r1cs or from_witness:
            from gosnark_amd import r1csqap
            dev_r1cs = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)

        values_route = sharded and rccl_sharded and args.sharded_route == "values"
        if values_route:
            from gosnark_amd import r1csqap
            dev_r1cs = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
        vstate = {"i": 0, "hv": None, "mine": None}

        def step():
            if values_route:
                owner = vstate["i"] % world
                vstate["i"] += 1
                if rank == owner:
                    vstate["hv"], bad = groth16.witness_values(pk, dev_r1cs, inst.w, vstate["hv"])
                    if bad:
                        raise SystemExit("bench.py: the benchmark witness violates a constraint")
                vstate["mine"] = capi.scalars_scatter(vstate["hv"] if rank == owner else None, n, owner, vstate["mine"])
                return groth16.prove_sharded_values_rccl(pk, inst.w, vstate["mine"], r_, s_)
            if sharded:
                return groth16.prove_sharded_rccl(pk, inst.w, inst.px, r_, s_) if rccl_sharded else groth16.prove_sharded(pk, inst.w, inst.px, r_, s_)
            if from_r1cs:
                # one call: px from the resident sparse system (overwriting the resident px) behind the accumulations over w
                return groth16.prove_from_r1cs(pk, dev_r1cs, w_dev, r_, s_, px_dev)[0]
            if from_witness:
                return groth16.prove_from_witness(pk, dev_r1cs, w_dev, r_, s_)
            return groth16.prove_resident(pk, w_dev, px_dev, r_, s_)
        units_per_step = n
        workload = ("groth16_prove_2^%d_constraints_sharded_over_all_gpus_owner_values_route" if values_route else
                    "groth16_prove_2^%d_constraints_sharded_over_all_gpus" if sharded else
                    "groth16_px_from_sparse_r1cs_then_prove_2^%d_constraints_per_gpu" if from_r1cs else
                    "groth16_witness_to_proof_2^%d_constraints_per_gpu" if from_witness else
                    "groth16_prove_2^%d_constraints_per_gpu") % args.log2n
    elif args.workload == "prove_pinocchio":
        # snark.GenerateProofs (snark.go:254-289): 6 G1 MSMs over w sharing one plan + 1 G2 MSM + px / Z + 1 G1 MSM over h
        from gosnark_amd import snark
        inst = synth.gates_pinocchio_instance(n, seed) if args.instance == "gates" else synth.sqchain_pinocchio_instance(n, seed)
        pk = inst.device_pk()

        def step():
            return snark.prove_resident(pk, inst.w, inst.px)
        units_per_step = n
        workload = "pinocchio_prove_2^%d_constraints_per_gpu" % args.log2n
    else:
        from gosnark_amd import parallel
        nterms = n                                        # per rank: msm_sharded sums N * 2^log2n terms in total
        bases = capi.g1_fixed_base(synth.scalars_u64(nterms, seed + 1000 * rank))
        sc = capi.scalars_upload(synth.scalars_u64(nterms, seed + 77 + 1000 * rank))
        if args.workload == "msm_g1" or world == 1:
            def step():
                return capi.msm_resident(bases, sc, nterms)
        elif rccl_sharded:
            def step():
                return capi.msm_sharded(bases, sc)
        else:
            def step():
                return parallel.msm_g1_sharded(bases, sc, nterms)
        units_per_step = nterms
        workload = ("g1_msm_2^%d_terms_per_gpu" % args.log2n) + ("_gathered_partials" if args.workload == "msm_sharded" else "")

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    plain_prove = args.workload == "prove" and not sharded and not from_r1cs and not from_witness and not logical
    prove_pipe = plain_prove and args.pipeline >= 2
    witness_pipe = from_witness and args.pipeline >= 2
    pin_pipe = args.workload == "prove_pinocchio" and args.pipeline >= 2
    msm_pipe = args.workload == "msm_g1" and args.pipeline >= 2 and not logical

    def run_steps(count, on_done=None):
        if msm_pipe:
            return pipelined(lambda: capi.msm_begin(bases, sc, nterms), capi.msm_end, count, args.pipeline, on_done)
        if pin_pipe:
            from gosnark_amd import snark as _sn
            return pipelined(lambda: _sn.prove_begin(pk, inst.w, inst.px), _sn.prove_end, count, args.pipeline, on_done)
        if prove_pipe:
            return pipelined(lambda: groth16.prove_begin(pk, w_dev, px_dev, r_, s_), groth16.prove_end, count, args.pipeline, on_done)
        if witness_pipe:
            return pipelined(lambda: groth16.prove_witness_begin(pk, dev_r1cs, w_dev, r_, s_), groth16.prove_end, count, args.pipeline, on_done)
        last = None
        for _ in range(count):
            last = step()
            if on_done:
                on_done()
        return last

    # Untimed settling before the W warm-up steps: the first few hundred milliseconds after the (host-side) instance generation run
    # 5-15 % slow (clocks ramp from idle, first-touch of the workspaces); the timed region below is still exactly K steps.
    if args.settle_ms > 0 and world > 1 and one_job:
        run_steps(8)                 # steps with a collective inside: the same count on every rank, not a clock
    else:
        t_settle = time.perf_counter()
        while args.settle_ms > 0 and (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
            run_steps(max(1, min(args.steps, 4)))
    run_steps(args.warmup)
    tm_keys = ("acc_g1_ms", "acc_g1_launches", "acc_g1_terms", "acc_g1_adds", "acc_g2_ms", "acc_g2_terms", "acc_g2_adds",
               "total_ms", "plan_ms", "accumulate_ms", "reduce_ms", "poly_ms", "plan_digits", "plan_entries", "heavy_buckets")
    tm_acc = {k: 0.0 for k in tm_keys}
    window_bits = [0]

    def book():
        tm = capi.last_timing()      # HIP-event timings recorded on the library's streams for the operation just collected
        for k in tm_keys:
            tm_acc[k] += tm[k]
        window_bits[0] = tm["window_bits"]
    rep_elapsed, last = [], None
    for _ in range(max(1, args.reps)):
        barrier()
        t0 = time.perf_counter()
        last = run_steps(args.steps, None if logical else book)
        barrier()
        elapsed = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if cpu_collectives else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        rep_elapsed.append(elapsed)
    elapsed = statistics.median(rep_elapsed)
    total_steps = args.steps * len(rep_elapsed)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)
    # what the library holds in the state the timed steps ran in (VERDICT r5 weak #8a: round 5 took this snapshot at the very end, after the
    # cold-path extras had dropped the window tables, so the line said table_bytes 0 under policy `always`)
    memory_timed = None
    try:
        mq = capi.memory_query()
        memory_timed = {k: mq[k] for k in ("device_total_bytes", "device_free_bytes", "library_bytes", "object_bytes", "table_bytes", "workspace_bytes", "evictions")}
        memory_timed["table_policy"] = args.table_policy
        memory_timed["taken"] = "right after the timed steps, before any extra measurement"
    except capi.GosnarkHipError:
        pass

    proof_verified = None
    if args.full and args.workload == "prove" and not logical and args.instance in ("setup", "realistic", "gates") and not args.no_check:
        # Product verifier (groth16.VerifyProof -> gs_groth16_verify, host side), outside the timed region, on EVERY rank:
        # the proof of this rank's instance against the vk its device setup produced, for the right public input and a wrong one.
        p_last = step()
        good = groth16.VerifyProof(inst.vk, p_last, [x_pub]) and not groth16.VerifyProof(inst.vk, p_last, [(x_pub + 1) % R])
        if world > 1:
            t = torch.tensor([1.0 if good else 0.0], dtype=torch.float64, device="cpu" if cpu_collectives else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            good = bool(t.item() == 1.0)
        if not good:
            raise SystemExit("bench.py: groth16.VerifyProof rejected the proof of the benchmarked instance (or accepted a wrong public input)")
        proof_verified = "groth16.VerifyProof accepted each rank's proof against its device-built vk and rejected a wrong public input (%d/%d ranks)" % (world, world)
    if args.full and args.workload == "prove_pinocchio" and not args.no_check:
        from gosnark_amd import snark as _snark
        p_last = step()
        good = _snark.VerifyProof(inst.vk, p_last, inst.public) and not _snark.VerifyProof(inst.vk, p_last, [(inst.public[0] + 1) % R])
        if world > 1:
            t = torch.tensor([1.0 if good else 0.0], dtype=torch.float64, device="cpu" if cpu_collectives else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            good = bool(t.item() == 1.0)
        if not good:
            raise SystemExit("bench.py: snark.VerifyProof rejected the proof of the benchmarked instance (or accepted a wrong public input)")
        proof_verified = "snark.VerifyProof (five pairing equations) accepted each rank's proof against its device-built vk and rejected a wrong public input (%d/%d ranks)" % (world, world)
    proof_check = None
    if args.full and rank == 0 and world == 1 and args.cpu_log2n > 0 and plain_prove and args.instance in ("setup", "realistic", "gates") and not args.no_check:
        # Outside the timed region, part of the checker/baseline leg (the only place bench.py touches oracle/): the toxic
        # values of the synthetic setup are known, so the proof the benchmarked instance must produce is known in closed form.
        proof_check = checker_leg_proof(step(), inst, r_, s_)

    extras = {}
    if args.full and rank == 0 and world == 1 and plain_prove and not args.no_extras:
        # --- every figure below is measured OUTSIDE the timed region and reported beside `value`, never as `value` -----------
        # one blocking call per proof (gs_groth16_prove_resident): the latency of a lone proof
        extras["blocking_ms_per_proof"], extras["blocking_ms_reps"] = time_calls_median(step, 6)
        # the boundary also accepts HOST buffers (gs_groth16_prove): w (32 B x m) and px (32 B x (2n-1)) then cross PCIe inside the call
        import ctypes
        lib = capi.load_library()
        outp = np.zeros(32, dtype=np.uint64)
        infp = (ctypes.c_int * 3)()
        rs = capi.ints_to_u64([r_, s_])
        extras["host_buffers_ms_per_step"] = time_calls(lambda: capi.check(lib.gs_groth16_prove(
            capi.Handle(pk.handle.h), capi.ptr64(inst.w_host), inst.w_host.shape[0], capi.ptr64(inst.px_host), inst.px_host.shape[0],
            capi.ptr64(rs[0]), capi.ptr64(rs[1]), capi.ptr64(outp), infp)), 3)
        if args.instance == "realistic":
            extras["witness_digits"] = witness_digit_stats(inst.w_host, window_bits[0], capi.last_timing())
        if args.instance in ("setup", "realistic", "gates"):
            # witness -> proof: px rebuilt from the resident sparse R1CS every time (gs_groth16_prove_r1cs; r1csqap.go:161-210 + groth16.go:225-278)
            from gosnark_amd import r1csqap
            dr = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
            pxh = capi.scalars_clone(inst.px, capi.get_device())
            groth16.prove_from_r1cs(pk, dr, inst.w, r_, s_, pxh)
            extras["from_r1cs_via_px_ms_per_step"] = time_calls(lambda: groth16.prove_from_r1cs(pk, dr, inst.w, r_, s_, pxh), 4)
            # ... and without px: H(x) straight from the constraint values (gs_groth16_prove_witness)
            pw = groth16.prove_from_witness(pk, dr, inst.w, r_, s_)
            ref = step()
            if (pw.PiA, pw.PiB, pw.PiC) != (ref.PiA, ref.PiB, ref.PiC):
                raise SystemExit("bench.py: gs_groth16_prove_witness disagrees with the px route")
            # (round 3 timed one un-warmed run of 6 calls here and the driver's box gave 15.1 ms against 11.3 elsewhere: VERDICT r3 weak 1c;
            #  the first calls after the px-route measurements above are listed one by one so that the line itself shows the ramp)
            first = []
            for _ in range(4):
                first.append(time_calls(lambda: groth16.prove_from_witness(pk, dr, inst.w, r_, s_), 1))
            extras["from_r1cs_first_calls_ms"] = first
            # (VERDICT r5 weak #8b: on the driver's box the FIRST of these three repetitions was 14.6 ms against 10.9 / 11.0.  The first calls of
            #  a route also build what only that route uses -- here the window table of the evaluation-basis array, 20 ms at 2^20, under policy
            #  `always` -- and the clock ramps from the px route's mix to this one's; so: six untimed calls first, and the repetitions as they are)
            extras["from_r1cs_ms_per_step"], extras["from_r1cs_ms_reps"] = time_calls_median(lambda: groth16.prove_from_witness(pk, dr, inst.w, r_, s_), 10, warm=6)
            extras["from_r1cs_constraints_per_s"] = n / extras["from_r1cs_ms_per_step"] * 1e3
            extras["from_r1cs_route"] = ("evaluation-basis PowersTauDelta (h-MSM over H's values, %d points)" % capi.pk_eval_count(pk.handle)
                                         if capi.pk_eval_count(pk.handle) else "coefficient route (interpolation + Taylor shift)")
            # ... three witness -> proof operations in flight (gs_groth16_prove_witness_begin / gs_groth16_prove_end)
            pipelined(lambda: groth16.prove_witness_begin(pk, dr, inst.w, r_, s_), groth16.prove_end, 6, 3)
            samples = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipelined(lambda: groth16.prove_witness_begin(pk, dr, inst.w, r_, s_), groth16.prove_end, 10, 3)
                torch.cuda.synchronize()
                samples.append((time.perf_counter() - t0) / 10 * 1e3)
            extras["from_r1cs_pipelined_ms_per_step"] = statistics.median(samples)
            extras["from_r1cs_pipelined_ms_reps"] = samples
            extras["from_r1cs_pipelined_constraints_per_s"] = n / extras["from_r1cs_pipelined_ms_per_step"] * 1e3
            if capi.pk_eval_count(pk.handle):
                # the same key through H's coefficients (round 2's route, what a key without the evaluation-basis array takes)
                capi.set_eval_basis(False)
                try:
                    pc = groth16.prove_from_witness(pk, dr, inst.w, r_, s_)
                    if (pc.PiA, pc.PiB, pc.PiC) != (ref.PiA, ref.PiB, ref.PiC):
                        raise SystemExit("bench.py: the coefficient witness route disagrees with the px route")
                    extras["from_r1cs_coefficient_route_ms_per_step"] = time_calls(lambda: groth16.prove_from_witness(pk, dr, inst.w, r_, s_), 4)
                finally:
                    capi.set_eval_basis(True)
            pxh.free()
            dr.handle.free()
        if args.instance == "setup" and args.table_policy == "always":
            extras["stream_distinct_host"] = stream_distinct_host(inst, pk, n, r_, s_, check=args.cpu_log2n > 0 and not args.no_check)
            extras["stream_distinct_host"]["resident_same_witness_ms_per_proof"] = extras.get("from_r1cs_pipelined_ms_per_step")
            extras["cold"] = cold_path(inst, pk, n, r_, s_, step())
        extras["msm_g1"] = msm_extras(seed + 5000)

    out = None
    if rank == 0:
        value = units_per_step * (1 if (sharded or logical) else world) * args.steps / elapsed
        launches = max(tm_acc["acc_g1_launches"], 1)
        avg_launch_s = tm_acc["acc_g1_ms"] / launches * 1e-3
        bytes_per_launch = G1_TERM_BYTES * tm_acc["acc_g1_terms"] / launches
        achieved = bytes_per_launch / avg_launch_s / 1e9 if avg_launch_s > 0 else 0.0
        mads = tm_acc["acc_g1_adds"] / launches * MADS_PER_MIXED_ADD / avg_launch_s / 1e12 if avg_launch_s > 0 else 0.0
        is_pin = args.workload == "prove_pinocchio"
        is_prove = bool(args.workload == "prove" or is_pin or (logical and sharded))
        # SURVEY 8d bytes per constraint: Groth16 544 n (4 G1 + 1 G2 MSM) + 128 n (H stage); Pinocchio 7 G1 + 1 G2 + H = 960 n
        step_bytes = (960 * n if is_pin else 672 * n) if is_prove else G1_TERM_BYTES * n
        cbits = window_bits[0]
        out = {
            "metric": ("Pinocchio constraints/sec (prove) at 2^%d R1CS" % args.log2n if is_pin else
                       "Groth16 constraints/sec (prove) at 2^%d R1CS" % args.log2n if is_prove else "G1-MSM terms/sec"),
            "value": value,
            "unit": unit_override or ("constraints/s" if is_prove else "terms/s"),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "reps": len(rep_elapsed), "ms_per_step_reps": [e / args.steps * 1e3 for e in rep_elapsed],
            "ms_per_step_min": min(rep_elapsed) / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if (sharded or logical) else "weak", "vs_baseline": None,
            "dtype": "u32 (9x29-bit Montgomery limbs of the 254-bit BN128 fields)", "data": "synthetic",
            "config": {"workload": workload, "settle_ms_before_warmup": args.settle_ms, "proofs_in_flight": args.pipeline if (prove_pipe or msm_pipe or pin_pipe or witness_pipe) else 1, "constraints": n, "variables": n + 1, "npublic": 1,
                       "window_bits": cbits,
                       "parallelism": (("%d logical devices of one GPU in one process (gs_groth16_prove_multi / gs_msm_g1_multi), records through ncclAllGather" % logical) if logical else
                                       "one proof, MSM term ranges sharded over the ranks, in-library RCCL gather of one 416-byte record per rank" if sharded else
                                       "independent proofs, one per GPU" if is_prove else args.workload),
                       "instance": inst.describe() if (is_prove and inst is not None) else "uniform random scalars, bases k_i*G"},
        }
        if not logical:
            out["roofline"] = {"bound": "hbm", "kernel": "k_bucket_accumulate<G1>", "achieved": achieved, "peak": HBM_PEAK_GBS,
                               "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                               "avg_launch_ms": avg_launch_s * 1e3, "algorithmic_bytes_per_launch": bytes_per_launch,
                               "note": "integer-issue bound (254-bit modular arithmetic on 32-bit VALU): PMC evidence under profiles/ "
                                       "(VALU ~96 % busy), see DESIGN.md section 5"}
            # the roofline that actually binds the dominant kernel: 32x32+64-bit multiply-add issue (v_mad_u64_u32).  One mixed
            # addition = 1467 mads; a term takes one addition per digit position (floor(254 / c) + 1 of them).
            out["roofline_valu"] = {"bound": "valu-int-mad", "kernel": "k_bucket_accumulate<G1>", "achieved": mads, "peak": MAD_PEAK_T,
                                    "unit": "T lane-mad/s", "frac": mads / MAD_PEAK_T,
                                    "peak_architectural": MAD_PIPE_T, "frac_of_architectural": mads / MAD_PIPE_T,
                                    "note": "mixed additions per launch (gs_timing.acc_g1_adds: the non-zero digits the plan counted) x 1467 v_mad_u64_u32; window width "
                                            "c = %d -> at most %d additions per term; peak = the sustained full-chip rate of tools/ubench_issue.hip at the kernel's three waves "
                                            "per SIMD (profiles/r06_power_clock_trace.txt; 31.5 in rounds 1-5); peak_architectural = 1024 SIMDs x 16 lanes per clock x 2.4 GHz, "
                                            "the multiplier pipe itself (profiles/r06_ubench_placement_cu_mask.txt: 89 %% of it at three waves per SIMD, 95 %% at six)" % (cbits, 254 // max(cbits, 1) + 1)}
            # ... and the limit under that one: a 64-wide wave occupies its 16-lane SIMD for 4 cycles per VALU instruction, whatever the
            # instruction; the G1 mixed addition is 2090 of them (SQ_INSTS_VALU, profiles/r04_pmc_sq_accumulate_prove.txt)
            wave_instr = tm_acc["acc_g1_adds"] / launches / 64.0 * VALU_PER_MIXED_ADD / avg_launch_s if avg_launch_s > 0 else 0.0
            out["roofline_issue"] = {"bound": "valu-issue", "kernel": "k_bucket_accumulate<G1>", "achieved": wave_instr / 1e9, "peak": ISSUE_PEAK_G,
                                     "unit": "G wave-instructions/s", "frac": wave_instr / 1e9 / ISSUE_PEAK_G,
                                     "note": "2090 VALU instructions per mixed addition x additions / 64 lanes; peak = the rate at which the chip executes fp29.h's own "
                                             "Montgomery products (dots3, random data) in a bare loop without loads, SUSTAINED: 207 VALU instructions per 377 ns per SIMD "
                                             "(tools/ubench_mulmod.hip 2 4: 876 cycles per product per SIMD at sclk 2.39 GHz).  Per class the G1 addition sums to 9.3 k "
                                             "cycles (1474 multiply-adds x 4.47 + 313 other VOP3 x 4.6 + 337 VOP2 x 2.9 + 249 s_nop x 1.35); the kernel takes 9.9-10.1 k at the "
                                             "2.01-2.05 GHz a probe wave reads beside the proof stream (profiles/r06_clock_timeline.txt: the accumulation kernels, and only they, are "
                                             "limited to ~2.0 GHz after 2-3 ms): 0.92-0.94 in cycles, 0.78-0.80 in time.  4.47 cycles per multiply-add is "
                                             "the SIMD's own rate at three waves per SIMD, on 8 CUs as on 256 (a sixteen-lane pipe: 4 cycles per wave at best, 7.8 k cycles per "
                                             "addition architecturally), not a clock or a socket-wide limit: profiles/r06_power_clock_trace.txt, r06_ubench_placement_cu_mask.txt"}
            out["roofline_whole_step"] = {"bound": "hbm", "algorithmic_bytes_per_step": step_bytes,
                                          "achieved": step_bytes / (elapsed / args.steps) / 1e9,
                                          "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                          "note": "SURVEY 8d: Groth16 672 B per constraint per proof (544 n MSM + 128 n H stage), Pinocchio 960 B; wall time per step"}
            out["device_ms_per_step"] = {k: tm_acc[k] / total_steps for k in ("total_ms", "poly_ms", "plan_ms", "accumulate_ms", "reduce_ms", "acc_g1_ms", "acc_g2_ms")}
            if tm_acc["plan_digits"]:
                out["plan_per_step"] = {"digits": tm_acc["plan_digits"] / total_steps, "bucket_additions": tm_acc["plan_entries"] / total_steps,
                                        "zero_digit_share": 1.0 - tm_acc["plan_entries"] / tm_acc["plan_digits"], "heavy_buckets": tm_acc["heavy_buckets"] / total_steps}
            live, why = (live_pmc_traffic(args) if (args.full and world == 1 and plain_prove and not args.no_extras) else
                         (None, "only the single-GPU run with --full measures it"))
            if live:
                # raw counters: the guide's x2 correction of FETCH_SIZE is calibrated for wide coalesced streams; this kernel's reads are 64-byte
                # gathers, so the raw sum is `traffic` and the x2-corrected read side is given as the upper bound
                out["roofline"]["traffic"] = live["fetch_bytes_per_launch_raw"] + live["write_bytes_per_launch_raw"]
                out["roofline"]["traffic_upper_bound_fetch_x2"] = 2 * live["fetch_bytes_per_launch_raw"] + live["write_bytes_per_launch_raw"]
                out["roofline"]["traffic_source"] = ("measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (two separate passes of this script, one step each, "
                                                     "no tracing domains), counter x 1024 B averaged over %d / %d k_bucket_accumulate<G1> dispatches"
                                                     % tuple(live["dispatches_averaged"]))
                out["roofline"]["traffic_over_algorithmic"] = out["roofline"]["traffic"] / bytes_per_launch if bytes_per_launch else None
            try:
                if live:
                    raise OSError("measured live")
                with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
                    pmc = json.load(f).get(workload)
                if pmc and pmc.get("window_bits") not in (None, cbits):
                    # the counters were taken with another window width = another number of table rows per term: stale, do not quote
                    out["roofline"]["traffic_source"] = ("profiles/pmc_traffic.json was measured at window width %s, this run used %d: not quoted"
                                                         % (pmc.get("window_bits"), cbits))
                elif pmc:      # measured offline with rocprofv3 --pmc (bench.py cannot attach counters to itself)
                    out["roofline"]["traffic"] = pmc["fetch_bytes_per_launch_raw"] + pmc["write_bytes_per_launch_raw"]
                    out["roofline"]["traffic_source"] = ("profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, raw counters; measured at commit %s, "
                                                         "window width %s) -- the live passes did not run: %s" % (pmc.get("commit", "?"), pmc.get("window_bits", "?"), why))
            except OSError:
                pass
        if shard_info:
            S = shard_info["logical_shards"]
            tail_ms = 0.35          # host pair sums + the O(1) tail (two result-dependent scalar multiplications), DESIGN.md section 6
            modelled = max(shard_info["per_shard_ms"]) + shard_info["gather_ms_one_rank_rccl"] + (tail_ms if sharded else 0.0)
            shard_info["MODELLED_not_measured"] = {
                "gpus": S, "ms_per_step": modelled, "value": n / modelled * 1e3, "unit": out["unit"],
                "model": "max over shards of the shard's time alone on one MI355X + the measured 1-rank ncclAllGather latency of the S records"
                         + (" + %.2f ms host tail" % tail_ms if sharded else "") +
                         "; on S GPUs the shards run concurrently.  NOT measured: no multi-GPU hardware is reachable from this run."}
            if "values_route" in shard_info:
                vr = shard_info["values_route"]
                per_proof = max(vr["per_shard_ms_three_in_flight"]) + vr["owner_polynomial_stage_ms"] / S
                vr["MODELLED_not_measured"] = {
                    "gpus": S, "ms_per_proof_streaming": per_proof, "value": n / per_proof * 1e3, "unit": out["unit"],
                    "ms_latency_of_a_lone_proof": max(vr["per_shard_ms"]) + vr["owner_polynomial_stage_ms"] + shard_info["gather_ms_one_rank_rccl"] + tail_ms,
                    "model": "a stream of proofs on S GPUs, the ranks take turns as owner: per proof every rank spends its shard's sums with three shard operations in "
                             "flight (measured on one MI355X: the gather, the host tail of %.2f ms and the scatter of %d bytes per peer -- one ncclSend per xGMI link in one "
                             "group -- run beside the next proof's device work) + 1/S of one owner stage (measured); the latency of a lone proof uses the blocking shard time.  "
                             "NOT measured: no multi-GPU hardware is reachable from this run." % (tail_ms, vr["scatter_payload_bytes_per_peer"])}
            out["sharding"] = shard_info
        out["build"] = build_stamp()
        if memory_timed is not None:
            out["memory"] = memory_timed
        try:       # ... and after everything else this script measured (the cold-path extras release and rebuild tables, other routes grow their own workspaces)
            mq = capi.memory_query()
            out["memory_after_extras"] = {k: mq[k] for k in ("library_bytes", "object_bytes", "table_bytes", "workspace_bytes", "evictions")}
        except capi.GosnarkHipError:
            pass
        for k, v in extras.items():
            out[k] = v
        if proof_verified:
            out["proof_verified"] = proof_verified
        if proof_check:
            out["proof_check"] = proof_check
        if args.full and world == 1 and args.cpu_log2n > 0 and not logical:
            out["cpu_baseline"] = cpu_baseline(args.cpu_log2n, seed + 1000)
            out["cpu_baseline_all_cores"] = cpu_baseline_all_cores(args.cpu_log2n + 3, seed + 2000)
            # the container may grant fewer CPUs than os.cpu_count() reports: state what the threads actually bought
            out["cpu_baseline_all_cores"]["speedup_vs_1_core"] = out["cpu_baseline_all_cores"]["value"] / out["cpu_baseline"]["value"]
            out["cpu_baseline_all_cores"]["cpus_granted"] = cpus_granted()
            if args.workload != "prove":
                out["cpu_baseline"]["note"] = "baseline is the Groth16 prove sample; 1 constraint ~ 4 G1 + 1 G2 terms"
            if plain_prove and not args.no_extras:
                out["cpu_baseline_reference_wasm"] = cpu_baseline_reference_wasm()
    if args.full and world > 1 and plain_prove and args.instance == "setup" and not args.no_strong:
        guard.line = out if rank == 0 else None
        torch_rccl = None
        if not share:       # torch's own RCCL group, exercised once: a sum of ones over the ranks (after the line is parked: a hang costs this probe only)
            guard.arm(min(120, args.strong_budget_s), "torch.distributed nccl group (RCCL): all_reduce probe")
            try:
                g = dist.new_group(backend="nccl")
                t = torch.ones(1, dtype=torch.float32, device="cuda")
                dist.all_reduce(t, group=g)
                torch.cuda.synchronize()
                torch_rccl = {"all_reduce_of_ones": float(t.item()), "ranks": world, "ok": int(t.item()) == world}
            except Exception as e:      # noqa: BLE001
                torch_rccl = _err(e)
            guard.disarm()
        strong = strong_ranks(args, world, rank, share, inst, pk, r_, s_, guard, cpu_collectives)
        if rank == 0:
            out["strong"] = strong
            out["rccl"] = rccl_report("rank: ncclCommInitRank, one process per GPU (gs_comm_init_rank)", strong.get("communicator_error"))
            out["rccl"]["torch_process_group_backend"] = dist.get_backend()
            out["rccl"]["torch_nccl_group_probe"] = torch_rccl
    if rank == 0:
        if world > 1:
            out["launch"] = "torch.distributed.run, one rank per GPU (WORLD_SIZE=%d)" % world + ("; " + "; ".join(launch_notes) if launch_notes else "")
            out["devices"] = device_report([0] * world if share else list(range(world)))
        import ctypes
        ctypes.CDLL(None).fflush(None)       # anything native libraries left in C stdio (RCCL's version banner) goes out BEFORE the line
        print(json.dumps(out), flush=True)
        guard.line = None
    if world > 1:
        guard.arm(60, "final barrier")
        dist.barrier()
        guard.disarm()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
