#!/usr/bin/env python3
"""Where the wave slots' time goes in one launch of the encode kernel (instrumented build: make -C c-blosc_amd prof): every persistent wave
records the device's real-time clock at entry and exit, the cycles it spent inside encode_one_stream, inside shuffle_block_task and waiting
for a block's shuffle, and the tasks it took (k_encode.hip; the per-stream records of scripts/enc_phase.py come from the same launch).
Printed for one launch:
  * the grid, the waves that took no task at all, and when waves start and end (histograms over the launch, 5 % of its length per column);
  * the wave slots occupied over time;
  * resident time split into streams, shuffle tasks, waiting and dispatch (tickets, descriptors, calls);
  * per XCD: when its last expensive-plane stream (the queue's first pass, queue_order.h) ends, and when its last wave leaves; ramp and tail.
Entry, exit and the streams' ends are readings of the real-time clock (100 MHz, the same on every CU); the cycle counts are shader clocks
(s_memtime starts differently on every shader engine and orders nothing between two waves).
    LIB=path/to/instrumented.so CHUNKS=128 python scripts/enc_wave_time.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import DATASETS

spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py")); mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
mod.LIB_PATH = os.environ.get("LIB", os.path.join(ROOT, "c-blosc_amd", "libblosc_amd_prof.so"))
lib = mod.load()
nchunks = int(os.environ.get("CHUNKS", "128")); csz = 64 << 20
dname = os.environ.get("DATA", "bench19"); codec = os.environ.get("CODEC", "lz4").encode()
TS = int(os.environ.get("TYPESIZE", "8")); SHUF = int(os.environ.get("SHUFFLE", "1")); CLEVEL = int(os.environ.get("CLEVEL", "5"))
OUT = os.environ.get("PROFILE_FILE", "/tmp/encwaves.bin")
dev = torch.device("cuda:0")
cus = torch.cuda.get_device_properties(0).multi_processor_count
host = DATASETS[dname](csz)
src = torch.from_numpy(host).to(dev).unsqueeze(0).expand(nchunks, csz).contiguous()
comp = torch.empty((nchunks, csz + 16), dtype=torch.uint8, device=dev)
bc = mod.DeviceBatch([src[i].data_ptr() for i in range(nchunks)], [csz] * nchunks, [comp[i].data_ptr() for i in range(nchunks)], [csz + 16] * nchunks)
for _ in range(3):      # the third call runs in the queue order learnt from the two before, like the benchmark's timed steps
    bc.compress(TS, CLEVEL, SHUF, codec, 0)
os.environ["BLOSC_AMD_ENC_PROFILE"] = OUT
lib.blosc_gpu_profile(1); lib.blosc_gpu_profile_reset()
bc.compress(TS, CLEVEL, SHUF, codec, 0)
lib.blosc_gpu_profile(0)
del os.environ["BLOSC_AMD_ENC_PROFILE"]
ms, launches = mod.profile_get("k_zstd_encode" if codec == b"zstd" else "k_encode_streams")
S = np.fromfile(OUT, np.uint32).reshape(-1, 16)
W = np.fromfile(OUT + ".waves", np.uint32).reshape(-1, 16)
written = W[:, 11] == 1
print(f"{os.path.basename(mod.LIB_PATH)}: {dname} {codec.decode()} clevel {CLEVEL} typesize {TS}, {nchunks} x 64 MiB: kernel {ms / max(launches, 1):.3f} ms (instrumented), "
      f"ratio {csz / bc.results()[0]:.3f}")
print(f"grid {W.shape[0]} workgroups = {W.shape[0] / cus:.2f} per CU on {cus} CUs; records written {int(written.sum())}; streams {S.shape[0]}")
G = W.shape[0]
W = W[written].astype(np.int64)
t_in = W[:, 0] | (W[:, 1] << 32); t_out = W[:, 2] | (W[:, 3] << 32)      # real-time clock, 10 ns
xcc = W[:, 10]
res = W[:, 12].astype(np.float64)                                          # shader clocks from entry to exit
rt = (t_out - t_in).astype(np.float64)
T0 = int(t_in.min())
idle = W[:, 7] == 0
print(f"shader clock {res.sum() / max(rt.sum(), 1.0) * 100:.0f} MHz (resident cycles / resident time)")
print(f"waves that took no task: {int(idle.sum())} of {G} ({100.0 * idle.sum() / G:.1f} %, {idle.sum() / cus:.2f} per CU); tasks taken {int(W[:, 7].sum())} = {int(W[:, 8].sum())} streams + "
      f"{int((W[:, 7] - W[:, 8]).sum())} shuffle entries; shuffle tasks run {int(W[:, 9].sum())} ({int(W[:, 9].sum() - (W[:, 7] - W[:, 8]).sum())} of them by waiting waves)")

rel_in = (t_in - T0).astype(np.float64); rel_out = (t_out - T0).astype(np.float64)
span = np.array([rel_out[xcc == x].max() if (xcc == x).any() else 0.0 for x in range(8)])
L = span.max()
print(f"launch length (first entry to last exit): {L / 100:.0f} us; last exit per XCD: " + " ".join(f"{v / 100:.0f}" for v in span))
B = 20
edges = np.linspace(0, L, B + 1); edges[-1] += 1
h_in, _ = np.histogram(rel_in, edges); h_out, _ = np.histogram(rel_out, edges); hi_in, _ = np.histogram(rel_in[idle], edges)
print("\nwave starts and ends over the launch (columns: 5 % of its length each)")
print(" starts            " + " ".join(f"{v:5d}" for v in h_in))
print("  that took no task" + " ".join(f"{v:5d}" for v in hi_in))
print(" ends              " + " ".join(f"{v:5d}" for v in h_out))
mid = (edges[:-1] + edges[1:]) / 2
occ = np.array([((rel_in <= t) & (rel_out > t)).sum() for t in mid])
print(" resident (middle) " + " ".join(f"{v:5d}" for v in occ))
print(" per CU            " + " ".join(f"{v / cus:5.1f}" for v in occ))
print(f"mean resident waves over the launch: {rt.sum() / L:.0f} = {rt.sum() / L / cus:.2f} per CU = {100.0 * rt.sum() / L / (32 * cus):.1f} % of the CUs' 32 wave slots "
      f"(the grid asks for {100.0 * G / (32 * cus):.1f} %); the waves that took tasks alone: {rt[~idle].sum() / L / cus:.2f} per CU")

# the split of resident time
slot13 = float(S[:, 13].astype(np.float64).sum())
t_stream = float(W[:, 4].sum()) - slot13; t_shuf = float(W[:, 5].sum()); t_wait = float(W[:, 6].sum()) + slot13
t_res = float(res.sum()); t_disp = t_res - t_stream - t_shuf - t_wait
phases = float(S[:, 8:13].astype(np.float64).sum())
print("\nresident wave time, all waves (M shader clocks, share)")
for name, v in (("streams (encode_one_stream without its wait)", t_stream), ("  of that inside the encoders' phases (slots 8 - 12)", phases), ("shuffle tasks", t_shuf),
                ("waiting for a block's shuffle (queue loop + slot 13)", t_wait), ("  of that slot 13 (second poll, inside encode_one_stream)", slot13),
                ("  of that in front of a wave's first stream (the ramp)", float(W[:, 13].sum())),
                ("dispatch: tickets, descriptors, calls, entry and exit", t_disp), ("resident", t_res)):
    print(f" {name:58s} {v / 1e6:10.1f}  {100.0 * v / t_res:5.1f} %")
print(f" of grid x launch length: resident {100.0 * rt.sum() / (G * L):.1f} %, on task (streams + shuffle tasks) {100.0 * rt.sum() / (G * L) * (t_stream + t_shuf) / t_res:.1f} %")
nsh = max(int(W[:, 9].sum()), 1)
print(f" per task: stream {t_stream / max(int(W[:, 8].sum()), 1) / 1e3:.1f} k clocks, shuffle task {t_shuf / nsh / 1e3:.1f} k clocks, dispatch {t_disp / max(int(W[:, 7].sum()), 1) / 1e3:.2f} k clocks per task taken")

# the end of every XCD's first pass: the last stream of an expensive plane (more than half of the most expensive plane's mean cycles, queue_order.h: plane_order)
NP = TS if SHUF == 1 else 1
if NP > 1 and S.shape[0] % NP == 0:
    cyc = S[:, 8:13].astype(np.float64).sum(axis=1).reshape(-1, NP)
    mean = cyc.mean(axis=0)
    heavy = mean > mean.max() / 2
    ends = ((S[:, 15].astype(np.int64) - T0) & 0xFFFFFFFF).astype(np.float64).reshape(-1, NP)
    blk_x = np.arange(ends.shape[0]) % 8
    print(f"\nexpensive planes (first pass of the queues): {[int(i) for i in np.nonzero(heavy)[0]]}; mean k clocks per plane: " + " ".join(f"{v / 1e3:.0f}" for v in mean))
    print(" XCD  first pass ends  last stream ends  last wave leaves   (us after the launch's first entry)")
    for x in range(8):
        if (xcc == x).any():
            print(f" {x:3d}  {ends[blk_x == x][:, heavy].max() / 100:15.0f}  {ends[blk_x == x].max() / 100:16.0f}  {span[x] / 100:16.0f}")
work = ~idle
first_leave = rel_out[work].min()
tail = np.clip(L - rel_out[work], 0, None).sum()
print(f"tail: the first working wave leaves at {first_leave / 100:.0f} us = {100.0 * first_leave / L:.1f} % of the launch; slots empty behind leaving waves: "
      f"{100.0 * tail / (work.sum() * L):.1f} % of working waves x launch length")
ramp = rel_in[work]
print(f"ramp: working waves enter between {ramp.min() / 100:.0f} and {ramp.max() / 100:.0f} us (mean {ramp.mean() / 100:.0f}); slots empty in front of entering waves: "
      f"{100.0 * ramp.sum() / (work.sum() * L):.1f} % of working waves x launch length")
