#!/usr/bin/env python3
"""Where a right-hand side of the forward kernel spends its cycles: shader-clock stamps of ONE wave (workgroup 777 of the 4 096 x 241
benchmark launch, its SIMD partner and the rest of the chip running as usual) at six points of every evaluation.

    tools/build_variant.sh fwdtrace -DHODE_FWD_TRACE=777          (here)
    HODE_LIB=<...>/hode/lab/libhode_fwdtrace.so python tools/fwd_trace.py      (GPU box)

Prints, per segment, the mean cycles over the evaluations of the steady state and the cycles its vector instructions would take
at 4.2 pipe cycles each with two waves sharing the pipe (2 x 4.2 per instruction of THIS wave): the excess is stall.

    ... python tools/fwd_trace.py --lifetimes [--tape]

The LIFETIME of every wave of the launch instead (hode_rhs_eval.h, g_wl: entry, end of the weight prologue, grid index T/4, T/2, 3T/4,
exit, the hardware id of its slot), grouped by SIMD, for B = 2 048 (one round of the chip's wave slots) and 4 096 (the benchmark):
how far apart the partners of a SIMD finish, how long a SIMD runs one wave only, how long none before the launch ends, and the weight
prologue of each round.  HODE_LIB names the build, so a library built with -DHODE_FWD_NOPACE gives the picture without the pacing."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
import hode  # noqa: E402

dev = torch.device("cuda")


def lifetimes(tape):
    lib = C.CDLL(hode.lib_path())
    nn, ode = bench.synth_weights(0).to(dev), bench.ODE_DEFAULT.to(dev)
    print(f"wave lifetimes of the forward launch, lib {os.path.basename(hode.lib_path())}, tape={tape}")
    data = {}
    for B in (2048, 4096):
        x0, t, meal, tvns = (v.to(dev) for v in bench.synth_cohort(B, 1000))
        sol = hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, 64, 4, want_tape=tape)
        run = lambda: hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, 64, 4, want_tape=tape, tape=sol.tape if tape else None)  # noqa: E731
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            run()
        e1.record()
        torch.cuda.synchronize()
        buf = np.zeros(B * 8, np.uint64)
        rc = lib.hode_lab_fwd_lifetimes(buf.ctypes.data_as(C.c_void_p), C.c_int(B))
        assert rc == 0, rc
        data[B] = (e0.elapsed_time(e1) / 4, buf.reshape(B, 8))
        del sol
    mhz = None
    for B in (4096, 2048):
        ms, rec = data[B]
        assert np.array_equal(rec[:, 7] & np.uint64(0xffffffff), np.arange(B, dtype=np.uint64)), "a record is missing"
        st = rec[:, :6].astype(np.int64)                           # shader-clock stamps
        hw = (rec[:, 6] & np.uint64(0xffffffff)).astype(np.int64)
        xcc = (rec[:, 6] >> np.uint64(32)).astype(np.int64) & 15
        rt = (rec[:, 7] >> np.uint64(32)).astype(np.int64)         # 100 MHz, one counter for the chip, low word
        rt = (rt - rt.min()) & 0xffffffff
        # SIMD = XCC | SE, SH, CU (HW_ID bits 15:8) | SIMD (bits 5:4); the wave slot (bits 3:0) is not part of the key
        simd = (xcc << 16) | (hw & 0xff00) | ((hw >> 4) & 3)
        keys, inv, cnt = np.unique(simd, return_inverse=True, return_counts=True)
        if mhz is None:
            # the s_memtime counters of different CUs are not aligned, so stamps are only ever compared within a SIMD; their rate
            # comes from the two rounds of B = 4 096: exit cycles against exit real time (10 ns ticks) of a SIMD's first and last wave
            r = []
            for i in range(len(keys)):
                w = np.nonzero(inv == i)[0]
                a, b = w[np.argmin(st[w, 5])], w[np.argmax(st[w, 5])]
                if rt[b] - rt[a] > 20000:                          # exits more than 0.2 ms apart
                    r.append((st[b, 5] - st[a, 5]) / ((rt[b] - rt[a]) * 0.01))
            mhz = float(np.median(r))
        print(f"B={B}: launch {ms:.3f} ms (HIP events, mean of 4), {len(keys)} SIMDs on {len(np.unique(xcc))} XCCs hold waves, waves per SIMD "
              f"min {cnt.min()} / median {int(np.median(cnt))} / max {cnt.max()}, s_memtime ~{mhz:.0f} MHz (against s_memrealtime, B=4096)")
        us = lambda c: np.asarray(c, np.float64) / mhz  # noqa: E731
        keys, inv, cnt = np.unique(simd, return_inverse=True, return_counts=True)
        gap, lone, idle, ratio, pro = [], [], [], [], {1: [], 2: []}
        end_rt = rt.max()
        for i in range(len(keys)):
            w = np.nonzero(inv == i)[0]
            w = w[np.argsort(st[w, 0])]
            ent, ex = st[w, 0], st[w, 5]
            # resident waves over time: +1 at an entry, -1 at an exit
            ev = sorted([(int(c), 1) for c in ent] + [(int(c), -1) for c in ex])
            one = 0
            n = 0
            for (c, d), (c2, _) in zip(ev[:-1], ev[1:]):
                n += d
                if n == 1:
                    one += c2 - c
            lone.append(one)
            idle.append((end_rt - rt[w].max()) * 10.0 / 1e3)       # 10 ns ticks -> us
            if len(w) >= 2:
                last2 = np.sort(ex)[-2:]
                gap.append(last2[1] - last2[0])
                ratio.append((ex[0] - ent[0]) / max(1, ex[1] - ent[1]))       # first-dispatched pair: older / younger lifetime
            for r, j in enumerate(w):
                pro[1 if r < 2 else 2].append(st[j, 1] - st[j, 0])
        q = lambda v: f"mean {np.mean(v):8.1f}  median {np.median(v):8.1f}  p90 {np.percentile(v, 90):8.1f}  max {np.max(v):8.1f}"  # noqa: E731
        print(f"  SIMD partners finish apart (last two exits of a SIMD), us:   {q(us(gap))}")
        print(f"  a SIMD runs ONE wave only (entry of its first to exit of its last), us: {q(us(lone))}")
        print(f"  a SIMD runs NO wave before the launch ends (chip-wide last exit), us:   {q(idle)}")
        print(f"  lifetime of the older wave of a SIMD's first pair / its younger wave:   mean {np.mean(ratio):.3f}  min {np.min(ratio):.3f}  max {np.max(ratio):.3f}")
        for r in (1, 2):
            if pro[r]:
                print(f"  weight prologue of round {r} ({len(pro[r])} waves), us:                        {q(us(pro[r]))}")
        qs = us(np.diff(st[:, 1:6], axis=1))
        print(f"  quarters of a trajectory (prologue end -> T/4 -> T/2 -> 3T/4 -> exit), mean us: {np.round(qs.mean(0), 1).tolist()}")
        print(f"  first entry to last exit of the chip (s_memrealtime at exit, lifetimes in s_memtime): "
              f"{(rt.max() - (rt - us(st[:, 5] - st[:, 0]) * 100).min()) / 100:.1f} us; first exit to last exit {(rt.max() - rt.min()) / 100:.1f} us; "
              f"entries of round 1 spread over {(np.sort(rt - us(st[:, 5] - st[:, 0]) * 100)[min(B, 2048) - 1] - (rt - us(st[:, 5] - st[:, 0]) * 100).min()) / 100:.1f} us")


if "--lifetimes" in sys.argv:
    lifetimes("--tape" in sys.argv)
    sys.exit(0)

B = 4096
x0, t, meal, tvns = (v.to(dev) for v in bench.synth_cohort(B, 1000))
nn, ode = bench.synth_weights(0).to(dev), bench.ODE_DEFAULT.to(dev)
tape = "--tape" in sys.argv
for _ in range(2):
    sol = hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, 64, 4, want_tape=tape)
torch.cuda.synchronize()
lib = C.CDLL(hode.lib_path())
buf = np.zeros(4096 * 8, np.uint64)
cnt = C.c_uint(0)
rc = lib.hode_lab_fwd_trace(buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size), C.byref(cnt))
assert rc == 0, rc
rec = buf.reshape(4096, 8).astype(np.int64)
rec = rec[rec[:, 0] > 0]
rec = rec[np.argsort(rec[:, 0])]
gap = np.diff(rec[:, 0])
start = int(np.argmax(gap)) + 1 if gap.size and gap.max() > 1e6 else 0         # the second launch starts after the longest pause
rec = rec[start:]
print(f"lib {os.path.basename(hode.lib_path())}  tape={tape}  evaluations of workgroup 777 in the ring: {len(rec)} of 1448 (second launch)")
rec = rec[8:8 + (len(rec) - 8) // 6 * 6]            # drop the two start-up evaluations and the first step: whole steps from here on
seg = {
    "state broadcast + mechanistic terms (entry -> mech)": rec[:, 6] - rec[:, 0],
    "first layer 9 -> 64 (mech -> h1)": rec[:, 1] - rec[:, 6],
    "hidden layer 1": rec[:, 2] - rec[:, 1],
    "hidden layer 2": rec[:, 3] - rec[:, 2],
    "hidden layer 3": rec[:, 4] - rec[:, 3],
    "output layer + sum (h4 -> return)": rec[:, 5] - rec[:, 4],
    "return -> next entry (stage algebra; every 6th: error norm, controller, output row, next interval)": np.append(rec[1:, 0] - rec[:-1, 5], 0),
}
tot = 0
for name, d in seg.items():
    d = d[:-1]
    if "next entry" in name:
        d = np.append(d, d[-1])
        ok = d < 20000                                   # (a slot that was overwritten leaves a hole in the sequence)
        per = np.array([d[i::6][ok[i::6]].mean() for i in range(6)])
        d = d[ok]
        print(f"  {name}:\n      by position in the step: {np.round(per).astype(int).tolist()}  mean {d.mean():.0f}")
    else:
        print(f"  {name}: mean {d.mean():7.0f}  min {d.min():6d}  p90 {np.percentile(d, 90):7.0f}")
    tot += d.mean()
print(f"  total per evaluation {tot:.0f} cycles  (x 1448 evaluations = {tot * 1448 / 1e6:.2f} M cycles per trajectory)")
# evaluation-to-evaluation time along the trajectory (deciles): is the wave slower at the start or the end of the launch?
ent = rec[:, 0]
d = np.diff(ent)
d = d[d < 20000]
dec = np.array_split(d, 10)
print("  entry-to-entry cycles by decile of the trajectory:", [int(x.mean()) for x in dec])
