#!/usr/bin/env python3
"""In what granules does the device hand out LDS?  Asks the runtime (hipOccupancyMaxActiveBlocksPerMultiprocessor through
blosc_internal_enc_lz_occupancy; nothing is launched) how many one-wave workgroups of the LZ4 encode kernel stay resident on a CU with
0 .. 1536 bytes of dynamic LDS on top of the kernel's own, and prints the table, then the persistent grids the engine uses
(blosc_internal_persistent_grids).  The output is profiles/r07b_lds_granule.txt; LDS_GRANULE_BYTES (enc_lz.h) quotes it.
    python scripts/lds_granule.py [STATIC_LDS_BYTES]      (default 6400: the kernel's static LDS, .group_segment_fixed_size of its code object)"""
import ctypes as C
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
try:
    import torch      # torch first where it is installed: it brings its own HIP runtime (bench.py)
    torch.cuda.init()
except Exception:
    pass
spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
mod = importlib.util.module_from_spec(spec)
sys.modules["c_blosc_amd"] = mod
spec.loader.exec_module(mod)
lib = mod.load()
static = int(sys.argv[1]) if len(sys.argv) > 1 else 6400
print(f"library: {mod.LIB_PATH}")
print(f"k_encode_streams_t<ENC_LZ>: {static} bytes of static LDS, 64 threads per workgroup")
print("dynamic LDS  total LDS  workgroups per CU  LDS if the total counts  LDS in 1280-byte granules")
prev = None
for dyn in range(0, 1536 + 1, 128):
    occ = lib.blosc_internal_enc_lz_occupancy(dyn)
    total = static + dyn
    gran = (total + 1279) // 1280 * 1280
    step = "" if prev is None or occ == prev else f"   <- steps from {prev}"
    print(f"{dyn:11d}  {total:9d}  {occ:17d}  {163840 // total:23d}  {163840 // gran:25d}{step}")
    prev = occ
lib.blosc_internal_persistent_grids.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
names, launched, occupancy = (C.c_char_p * 32)(), (C.c_int * 32)(), (C.c_int * 32)()
n = lib.blosc_internal_persistent_grids(32, names, launched, occupancy)
print("\npersistent kernel                     launched per CU  runtime occupancy")
for i in range(n):
    print(f"{names[i].decode():37s} {launched[i]:15d}  {occupancy[i]:17d}")
