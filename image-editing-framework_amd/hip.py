"""ctypes binding of `libief_hip.so` (C-ABI in `include/ief_hip.h`).

This is the ONLY route from the host code to compute: every function below launches a
hand-written gfx950 kernel on torch's current HIP stream, with torch tensors used purely as
device-memory handles (`data_ptr()`).  There is no CPU or eager-PyTorch fallback: if the library
is missing, or a tensor is not an fp16/fp32 device tensor of the documented layout, the call raises.

Nothing of the ABI is declared here by hand: the parameter structs, every entry point's `restype` /
`argtypes` and the header's constants are derived from `include/ief_hip.h` by `cabi.py`.
"""
import collections
import ctypes
import os
from ctypes import byref

import torch

from . import cabi

# IEF_HIP_LIB / IEF_PLAN_FILE: A/B two builds of the library (and their tuned tables) on one GPU box
ABI_VERSION = cabi.defines["IEF_ABI_VERSION"]
REPEAT_MAX_JOBS = cabi.defines["IEF_REPEAT_MAX_JOBS"]
_LIB_PATH = os.environ.get("IEF_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libief_hip.so")
_lib = None


class HipExtensionMissing(RuntimeError):
    pass


# the parameter blocks callers fill in: the very classes the entry points' POINTER(...) argtypes name
IefGemmParams = cabi.structs["IefGemmParams"]
IefAttnParams = cabi.structs["IefAttnParams"]
IefCrossParams = cabi.structs["IefCrossParams"]
IefGemmF32Params = cabi.structs["IefGemmF32Params"]
IefAttnF32Params = cabi.structs["IefAttnF32Params"]
IefRepeatJob = cabi.structs["IefRepeatJob"]
IefGemmX3pParams = cabi.structs["IefGemmX3pParams"]
IefAttnBwdParams = cabi.structs["IefAttnBwdParams"]
IefAttnBwdF32Params = cabi.structs["IefAttnBwdF32Params"]
IefMapLossParams = cabi.structs["IefMapLossParams"]


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load the shared library (once).  Raises HipExtensionMissing when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipExtensionMissing(
            f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C image-editing-framework_amd/csrc`).  There is no CPU fallback."
        )
    lib = ctypes.CDLL(_LIB_PATH)
    for name, (restype, argtypes) in cabi.functions.items():
        fn = getattr(lib, name)  # AttributeError here = header / library mismatch
        fn.restype, fn.argtypes = restype, argtypes
    if os.environ.get("IEF_X3_WIDE"):          # A/B runs: bit 0 clear = keep every launch on the 128 x 80 tile; bit 1 set = 32-key flash tiles
        lib.ief_gemm_x3_set_variant(int(os.environ["IEF_X3_WIDE"]))
    if lib.ief_abi_version() != ABI_VERSION:
        raise HipExtensionMissing("libief_hip.so ABI version mismatch; rebuild")
    for which, st in ((0, IefGemmParams), (1, IefAttnParams), (2, IefCrossParams), (3, IefAttnBwdParams), (4, IefMapLossParams),
                      (5, IefGemmF32Params), (6, IefAttnF32Params), (7, IefGemmX3pParams)):
        if lib.ief_struct_size(which) != ctypes.sizeof(st):
            raise HipExtensionMissing(f"{st.__name__}: ctypes layout ({ctypes.sizeof(st)} B) != library "
                                      f"({lib.ief_struct_size(which)} B); rebuild libief_hip.so")
    _lib = lib
    return lib


_ERR = {-1: "IEF_EINVAL (null / missing pointer)", -2: "IEF_ESHAPE (unsupported shape)", -3: "IEF_EALIGN (alignment)"}


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {_ERR.get(rc, f'hipError {rc}')}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------- live kernel timing
# bench.py brackets individual launches with HIP events ON THE STREAM THE KERNEL RUNS ON to get the
# dominant kernel's average launch duration (roofline.achieved).  Off by default (zero overhead).
_prof = None
PROF_SHAPES = os.environ.get("IEF_PROF_SHAPES", "0") == "1"     # append MxNxK to the timed kernel names (tests/exp_shapes.py)
# tile id -> (BM, BN, WAVES_M, WAVES_N), as in csrc/gemm_conv.hip
_TILES = {1: (128, 128, 2, 2), 2: (64, 128, 2, 2), 3: (64, 64, 2, 2), 4: (128, 64, 2, 2), 5: (64, 160, 2, 2),
          6: (128, 160, 2, 2), 7: (128, 160, 4, 2), 8: (256, 128, 4, 2), 9: (128, 128, 4, 2),
          14: (256, 80, 8, 1), 15: (256, 80, 8, 1),
          16: (128, 160, 4, 2), 17: (128, 128, 4, 2), 18: (256, 128, 4, 2), 19: (64, 160, 2, 2), 20: (64, 64, 2, 2),
          21: (128, 160, 2, 2)}
_TILE_NL = {16: 4, 17: 4, 18: 4, 19: 2, 20: 2, 21: 2}   # loader waves of a tile (csrc/gemm_conv.hip, NL): they stage, the others multiply
_HALO_TILES = (14, 15)  # conv3x3_halo_kernel (csrc/gemm_conv.hip): 3x3 / stride 1 / pad 1 convolutions only, rows of <= 64 pixels; 15: + 4 loader waves


def _kname(tile, conv, stages=2):
    bm, bn, wm, wn = _TILES[tile]
    if tile in _HALO_TILES:
        return f"conv3x3_halo_kernel<{bm}, {bn}, {wm}, {wn}, {4 if tile == 15 else 0}>"
    return f"igemm_f16_kernel<{bm}, {bn}, {wm}, {wn}, {stages or 2}, {_TILE_NL.get(tile, 0)}, {'true' if conv else 'false'}>"


def _ring_bytes(tile, stages):
    bm, bn, wm, wn = _TILES[tile]
    if tile in _HALO_TILES:         # fixed LDS image (two super-tile buffers + a 4-slot weight ring); one "ring depth"
        return 155776 if stages == 4 else 1 << 30
    rp = 64 * (_TILE_NL.get(tile, 0) or wm * wn) // 8
    rows = -(-bm // rp) * rp + -(-bn // rp) * rp
    return 2 * stages * rows * 64


_prof_staged = None      # kernel name -> bytes its launches staged into LDS by LDS-DMA since profile_begin (the planes kernels report them)


def profile_begin():
    global _prof, _prof_staged
    _prof = []
    _prof_staged = {}


def note_staged(name: str, nbytes: float):
    """a planes kernel's launch reports the bytes it moves L2 -> LDS (both operands, both planes, every K tile of every output tile):
    what the per-CU LDS-DMA fill rate prices"""
    if _prof is not None and _prof_staged is not None:
        _prof_staged[name] = _prof_staged.get(name, 0.0) + nbytes


def profile_staged():
    """{kernel name: LDS-staged bytes} of the launches since the last profile_begin"""
    return dict(_prof_staged or {})


def profile_end(with_bytes=False):
    """-> list of (kernel_name, algorithmic_flops, milliseconds[, algorithmic_bytes])"""
    global _prof
    rec, _prof = _prof, None
    torch.cuda.synchronize()
    if with_bytes:
        return [(name, flops, e0.elapsed_time(e1), nbytes) for name, flops, nbytes, e0, e1 in rec]
    return [(name, flops, e0.elapsed_time(e1)) for name, flops, nbytes, e0, e1 in rec]


class _Timed:
    """`nbytes`: the launch's ALGORITHMIC HBM traffic (every operand read once, the output written once)"""

    def __init__(self, name, flops, nbytes=0.0):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if _prof is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())

    def __exit__(self, *a):
        if _prof is not None:
            self.e1.record(torch.cuda.current_stream())
            _prof.append((self.name, self.flops, self.nbytes, self.e0, self.e1))


# GroupNorm statistics from the producer: a conv / 1x1-projection launch whose output is an NHWC activation of a level with
# at least this many pixels per image can leave per-tile column sums next to it (`col_stats=True` -> `(out, ColStats)`);
# the caller hands that object to the `groupnorm` that consumes the output (`cstat=` / `cstat2=`), which then folds the
# sums instead of running its own statistics pass.  The hand-off is an explicit value travelling beside the tensor it
# describes: nothing is attached to tensor objects, so a buffer re-written by any other launch cannot be paired with
# statistics of its earlier contents unless the caller itself keeps passing the old object.
GN_CSTAT = os.environ.get("IEF_GN_CSTAT", "1") == "1"
HALO_HEURISTIC = os.environ.get("IEF_HALO_HEURISTIC", "1") == "1"   # untuned plain 3x3 convolutions take the halo kernel
_CSTAT_MIN_HW = 256


class ColStats:
    """(sum, sum of squares) per M tile and output channel of ONE launch's fp16 output (IefGemmParams.cstat_out)"""
    __slots__ = ("buf", "bm", "hw", "ptr", "numel")

    def __init__(self, buf, bm, hw, out):
        self.buf, self.bm, self.hw = buf, bm, hw
        self.ptr, self.numel = out.data_ptr(), out.numel()

    def describes(self, t) -> bool:
        return t.data_ptr() == self.ptr and t.numel() == self.numel


def _attach_cstat(lib, p, out, M, N, hw):
    """decide whether this launch emits column statistics; returns the ColStats (owning the scratch tensor) or None"""
    if not GN_CSTAT or hw is None or hw < _CSTAT_MIN_HW or (p.splits > 1 and not p.cnt) or (p.flags & 2) or AUTOTUNE:
        return None
    bm = lib.ief_gemm_tile_bm(p.tile_hint)
    if bm <= 0 or hw % bm or M % hw:
        return None
    cs = torch.empty(M // bm, N, 2, dtype=torch.float32, device=out.device)
    p.cstat_out = cs.data_ptr()
    return ColStats(cs, bm, hw, out)


def pick_tile(M: int, N: int, batch: int = 1) -> int:
    """tile choice (mirrors dispatch_igemm in csrc/gemm_conv.hip): fill the 256 CUs"""
    nblk = lambda bm, bn: -(-M // bm) * -(-N // bn) * batch
    if nblk(128, 128) >= 384:
        return 1
    if nblk(64, 128) >= 256:
        return 2
    return 3


_zero_pages = {}   # device zero page: source of padded / out-of-range chunks for the LDS-DMA staging


def _zeros(device):
    z = _zero_pages.get(device)
    if z is None:
        z = _zero_pages[device] = torch.zeros(128, dtype=torch.float16, device=device)
    return z.data_ptr()


# ---- split-K arrival counters (IefGemmParams.cnt): one zeroed int per output tile, zero again when the launch ends.
# Launches that can overlap must not share counters, so:
#   eager launches   take the next slots of a ring of 2^20 ints per device (thousands of launches deep: a launch has ended
#                    long before its slots come round again);
#   captured launches take slots of an ARENA its owner allocated for that graph (`counter_arena`): a captured step graph
#                    keeps its own counters for as long as it lives, whatever other graphs or eager launches do; without an
#                    arena a captured launch falls back to the separate reducer launch.
SPLITK_INLAUNCH = os.environ.get("IEF_SPLITK_INLAUNCH", "1") == "1"
# ... and only where the last arriver's serial read stays short: splits x tile bytes (fp32) at most this many KiB.  Measured
# (same box, SD1.5 batch-4 step): combining EVERY split-K launch in the launch took the step from 7.45 to 7.97 ms — the
# tuned plans cut K 2-16 ways over 64..256-row tiles, 128 KiB - 1.3 MiB per output tile, which one workgroup reads at
# ~100 GB/s while the reducer launch reads with the whole chip (the guide's splitk-seam verdict).
SPLITK_INLAUNCH_MAX_KB = int(os.environ.get("IEF_SPLITK_INLAUNCH_MAX_KB", "64"))
_CNT_RING = 1 << 20
_cnt_ring = {}          # device -> [tensor, position]
_cnt_arena = None       # [tensor, position] while a capture that owns one is running
_cnt_used = 0           # ints handed out so far (owners size their arena by the delta over a warm-up pass)


def counters_used() -> int:
    return _cnt_used


class counter_arena:
    """`with counter_arena(n, device) as arena:` — split-K launches captured inside take their arrival counters from
    `arena` (a zeroed int32 tensor the caller keeps alive with the graph)"""

    def __init__(self, n, device):
        if isinstance(device, int):
            device = torch.device("cuda", device)
        self.t = torch.zeros(max(int(n), 1), dtype=torch.int32, device=device)

    def __enter__(self):
        global _cnt_arena
        self.prev, _cnt_arena = _cnt_arena, [self.t, 0]
        return self.t

    def __exit__(self, *a):
        global _cnt_arena
        _cnt_arena = self.prev


def _splitk_counters(device, n, combine_kb=0):
    """device pointer of n zeroed ints for one split-K launch, or None (-> separate reducer launch)"""
    global _cnt_used
    if not SPLITK_INLAUNCH or combine_kb > SPLITK_INLAUNCH_MAX_KB:
        return None
    if _capturing():
        if _cnt_arena is None or _cnt_arena[1] + n > _cnt_arena[0].numel():
            return None
        t, pos = _cnt_arena
        _cnt_arena[1] = pos + n
        _cnt_used += n
        return t.data_ptr() + 4 * pos
    ring = _cnt_ring.get(device)
    if ring is None:
        ring = _cnt_ring[device] = [torch.zeros(_CNT_RING, dtype=torch.int32, device=device), 0]
    if n > _CNT_RING:
        return None
    if ring[1] + n > _CNT_RING:
        # wrap: the slots about to be re-used may belong to launches of OTHER streams that have not run yet, and a launch
        # that faulted (or an exception between two ticket draws) leaves non-zero counters behind -- wait for the device and
        # zero the ring before handing its start out again (once per ~_CNT_RING counters: not on the hot path, which is the
        # captured graph with its own arena)
        reset_counters(device)
    ptr = ring[0].data_ptr() + 4 * ring[1]
    ring[1] += n
    _cnt_used += n
    return ptr


def reset_counters(device=None):
    """zero the eager split-K arrival-counter ring(s) after a device sync -- on wrap, and for callers recovering from a failed
    launch (a faulted kernel leaves its tickets drawn: every later launch re-using those slots would combine too early or never)"""
    for dev, ring in _cnt_ring.items():
        if device is None or dev == device:
            torch.cuda.synchronize(dev)
            ring[0].zero_()
            ring[1] = 0


def _tile_count(lib, tile_hint, M, N, splits=1):
    """(output tiles, KiB the last arriver of a tile would read: splits x BM x BN fp32)"""
    bm, bn = lib.ief_gemm_tile_bm(tile_hint), lib.ief_gemm_tile_bn(tile_hint)
    if bm <= 0 or bn <= 0:
        return 0, 0
    return -(-M // bm) * -(-N // bn), splits * bm * bn * 4 // 1024


SPLITK = os.environ.get("IEF_SPLITK", "1") != "0"
_SPLIT_TARGET = int(os.environ.get("IEF_SPLIT_TARGET", "512"))   # blocks wanted on the 256 CUs
_SPLIT_MAX = int(os.environ.get("IEF_SPLIT_MAX", "16"))
_SPLIT_MIN_KT = int(os.environ.get("IEF_SPLIT_MIN_KT", "6"))     # K tiles (of 64) each slice keeps at least

# ---- plan selection: tuned table first, heuristic otherwise -----------------------------------------
# `tuned_plans.json` (next to this file) maps "conv|M|N|K" / "gemm|M|N|K" -> [tile, splits]; it is produced
# on the GPU by `autotune_plan` (tests/tune_plans.py) and covers the SD1.5 layer shapes at batch 1 / 2 / 4.
_PLAN_FILE = os.environ.get("IEF_PLAN_FILE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_plans.json")
_plans = None
AUTOTUNE = os.environ.get("IEF_AUTOTUNE", "0") == "1"   # tune unseen shapes on first use (outside graph capture)


def read_plans(path):
    """{key: tuple} of a plan file (this module's and planes.py's); empty without the file or under IEF_NO_PLAN_TABLE=1"""
    if not os.path.exists(path) or os.environ.get("IEF_NO_PLAN_TABLE", "0") == "1":
        return {}
    import json
    with open(path) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def write_plans(path, table):
    import json
    with open(path, "w") as f:
        json.dump({k: list(v) for k, v in sorted(table.items())}, f, indent=0)


def _plan_table():
    global _plans
    if _plans is None:
        _plans = read_plans(_PLAN_FILE)
    return _plans


def save_plans(path=None):
    write_plans(path or _PLAN_FILE, _plan_table())


def heuristic_plan(M: int, N: int, K: int):
    """(tile, splits) without measurements.  SD channel widths are multiples of 320 = 2 x 160, so 160-wide
    tiles waste nothing on N; layers whose M x N alone gives too few tiles (the 32x32 .. 8x8 UNet levels, K up to
    23040) are cut along K until ~512 blocks exist, each slice keeping >= 6 K tiles of 64."""
    nk = -(-K // 64)
    if N % 160 == 0 and M >= 128:
        t6 = -(-M // 128) * (N // 160)
        if t6 >= 192 and (nk < 24 or t6 >= 384):
            return 7, 1
        if nk >= 12 and SPLITK:
            splits = max(1, min(-(-_SPLIT_TARGET // t6), nk // _SPLIT_MIN_KT, _SPLIT_MAX))
            if t6 * splits >= 128:
                return 6, splits
    t128 = -(-M // 128) * -(-N // 128)
    if not SPLITK or t128 >= 384 or nk < 24:
        return pick_tile(M, N), 1
    tile, tiles = 1, t128
    if M <= 64 or (tiles < 32 and M < 128):
        tile, tiles = 2, -(-M // 64) * -(-N // 128)
    splits = min(-(-_SPLIT_TARGET // tiles), nk // _SPLIT_MIN_KT, _SPLIT_MAX)
    if splits <= 1:
        return pick_tile(M, N), 1
    return tile, splits


# ---- plans that do not follow the batch ---------------------------------------------------------------
# Tile, split-K count and kernel family of the fp16-storage front-end follow M = batch rows x tokens, and another split count sums K in
# another order: the same row gives other last bits (of fp16 roundings) in a launch of another batch.  Inside `plans_per_row(rows)` a
# launch whose M is a multiple of `rows` is planned as ONE of its rows is planned (M / rows): every row then runs the arithmetic of a
# batch-1 launch whatever the batch.  The plan is that of the small shape, so this costs speed; for passes whose result must not
# depend on how their rows are chunked over launches (`DiffEdit.infer_mask`).
_PLAN_ROWS = 1


class plans_per_row:
    def __init__(self, rows: int):
        if not isinstance(rows, int) or rows < 1:
            raise ValueError(f"plans_per_row: rows must be a positive integer, got {rows!r}")
        self.rows = rows

    def __enter__(self):
        global _PLAN_ROWS
        self.saved, _PLAN_ROWS = _PLAN_ROWS, self.rows
        return self

    def __exit__(self, *exc):
        global _PLAN_ROWS
        _PLAN_ROWS = self.saved
        return False


def _plan_m(M: int) -> int:
    """the M a launch of M rows is planned for (`plans_per_row`)"""
    return M // _PLAN_ROWS if _PLAN_ROWS > 1 and M % _PLAN_ROWS == 0 else M


def pick_plan(M: int, N: int, K: int, conv: bool = False, variant: str = ""):
    """(tile, splits, stages); `variant` ("|u": the convolution with the fused nearest-2x upsample) has its own table key
    and falls back to the plain key of the same (M, N, K)"""
    kind = "conv" if conv else "gemm"
    hit = _plan_table().get(f"{kind}|{M}|{N}|{K}{variant}") if variant else None
    if hit is None:
        hit = _plan_table().get(f"{kind}|{M}|{N}|{K}")
    if hit is None:
        hit = heuristic_plan(M, N, K)
    return (hit[0], hit[1], hit[2] if len(hit) > 2 else 2)


def candidate_plans(M: int, N: int, K: int, conv: bool = False):
    nk = -(-K // 64)
    out = []
    for t, (bm, bn, _, _) in _TILES.items():
        if t in _HALO_TILES and not conv:
            continue
        for s in (1, 2, 4, 8, 16):
            blocks = -(-M // bm) * -(-N // bn) * s
            if s > 1 and (nk // s < 4 or blocks > 2048):
                continue
            if blocks < 48 and s < 16:
                continue
            for st in (2, 3, 4):
                if _ring_bytes(t, st) <= 160 * 1024 and (st == 2 or nk // s >= st):
                    out.append((t, s, st))
    return out


def _time_graph(fn, iters=20):
    """us per call of fn(i), i = 0..iters-1, replayed from one hipGraph"""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    used0 = counters_used()
    with torch.cuda.stream(st):
        fn(0)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    arena = counter_arena((counters_used() - used0) * iters, torch.cuda.current_device())   # split-K combines in the launch
    g = torch.cuda.CUDAGraph()
    with arena, torch.cuda.graph(g):
        for i in range(iters):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _cold_copies(w, iters=20, budget=320 << 20):
    """enough clones of a weight tensor that consecutive launches never find it in the 256 MiB Infinity Cache —
    inside the UNet every layer's weights stream from HBM once per step, which is what the tuner must see"""
    k = max(1, min(iters, -(-budget // max(1, w.numel() * w.element_size()))))
    return [w] + [w.clone() for _ in range(k - 1)]


def autotune_plan(kind: str, M: int, N: int, K: int, run, variant: str = ""):
    """time run(tile, splits, stages, i) for every candidate plan (hipGraph of 20 launches each, launch i using
    the i-th cache-cold weight copy); remember the best"""
    best = None
    for t, sp, st in candidate_plans(M, N, K, conv=(kind == "conv")):
        try:
            us = _time_graph(lambda i: run(t, sp, st, i))
        except RuntimeError:
            continue
        if best is None or us < best[0]:
            best = (us, t, sp, st)
    if best is not None:
        _plan_table()[f"{kind}|{M}|{N}|{K}{variant}"] = (best[1], best[2], best[3])
    return best


def _capturing() -> bool:
    return torch.cuda.is_current_stream_capturing()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev16(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16):
        raise TypeError(f"{name}: expected an fp16 device tensor, got "
                        f"{type(t).__name__ if not isinstance(t, torch.Tensor) else (t.dtype, t.device)}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: last dimension must be contiguous")
    return t


# How the contractions of the fp32-storage modes run (csrc/exact_f32.hip, csrc/split_x3.hip):
#   "f32"  the fp32-input MFMA (bitwise an fp32 fma chain; precision="f32")
#   "x3"   split operands: hi + lo fp16 halves of every fp32 element, three fp16 MFMAs per product (precision="f16x3")
# A model sets it for the duration of its own calls (`with hip.f32_contraction(mode)`): one Python thread drives the
# library, and a captured graph keeps the kernels that were chosen while it was recorded.
_F32_CONTRACT = "f32"
# powers of two.  Activations: 1 — the fp16 range itself (|x| < 65504, as on the fp16-storage path; a larger scale would narrow it:
# 4 capped activations at 16376) and the scale the pre-split operand planes carry (planes.py); gfx950's MFMA keeps fp16 subnormal
# inputs, so the lo half of a small element only loses ABSOLUTE resolution (2^-25), far below the 2^-22 relative error of the
# large elements that dominate a dot product.  Weights 2^8 (|w| < 255), softmax maps 2^14 (<= 1).
X3_SCALE_ACT, X3_SCALE_W, X3_SCALE_PROB = 1.0, 256.0, 16384.0


class f32_contraction:
    def __init__(self, mode: str):
        if mode not in ("f32", "x3"):
            raise ValueError('f32_contraction: mode must be "f32" or "x3"')
        self.mode = mode

    def __enter__(self):
        global _F32_CONTRACT
        self.saved, _F32_CONTRACT = _F32_CONTRACT, self.mode
        return self

    def __exit__(self, *exc):
        global _F32_CONTRACT
        _F32_CONTRACT = self.saved
        return False


# (data_ptr, shape, scale[, "phase"]) -> (weakref to the weight tensor, its _version, planes fp16 [2, N, K]; "phase": the phase form
# [2, 4, N, 4 C] of an Upsample2D weight, x3_upsample_phase_planes; a further tag "tiles": the same planes in the tiled order of
# ief_x3_tile_weights, x3_weight_tiles / x3_upsample_phase_tiles, kept BESIDE the row-major ones).  The entry dies WITH the weight
# (weakref.finalize): a model that is dropped frees its planes (they are as large as the weights).  A captured graph bakes the
# planes' address in: an in-place update of a weight after capture would replace the entry and free planes the graph still
# reads, so weights are immutable once a graph over them exists (the weight broadcast runs before any forward).
_x3_planes = {}
X3_FUSE_GEGLU = os.environ.get("IEF_X3_FUSE_GEGLU", "1") == "1"   # 0: FF1 writes its pre-activation, ief_geglu_il_f32 follows (A/B)
X3_PRESPLIT = os.environ.get("IEF_X3_PRESPLIT", "1") == "1"       # 0: split the weights in every launch, like the activations


def x3_weight_planes(w, scale=None):
    """the pre-split fp16 planes [2, N, K] of an fp32 WEIGHT tensor (hi = fp16(s w), lo = fp16(s w - hi)), made once per tensor
    and kept: a weight is static, so splitting it in every launch and workgroup would spend vector instructions the GEMM's
    steady-state loop has none to spare of.  None while a graph is being captured and the planes do not exist yet."""
    scale = X3_SCALE_W if scale is None else scale
    key = (w.data_ptr(), tuple(w.shape), float(scale))
    hit = _x3_planes.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version:
        return hit[2]
    if _capturing() or w.numel() % 4 or not w.is_contiguous():
        return None
    lib = load()
    n = w.shape[0]
    planes = torch.empty(2, n, w.numel() // n, dtype=torch.float16, device=w.device)
    _check(lib.ief_x3_split_weights(w.data_ptr(), planes.data_ptr(), w.numel(), float(scale), _stream()), "ief_x3_split_weights")
    import weakref
    _x3_planes[key] = (weakref.ref(w), w._version, planes)
    weakref.finalize(w, _x3_planes.pop, key, None)
    return planes


def x3_upsample_phase_planes(w, scale=None):
    """the PHASE form of an Upsample2D weight [Cout, 3, 3, C] as fp16 planes [2, 4, Cout, 4 C] (`ief_x3_upsample_phase_weights`:
    nearest-2x + 3x3 is four 2x2 convolutions of the low-resolution image whose taps are sums of the nine).  Cached per weight
    tensor exactly as `x3_weight_planes` (its own key: a layer that runs the phase form never creates the 9-tap planes)."""
    scale = X3_SCALE_W if scale is None else scale
    key = (w.data_ptr(), tuple(w.shape), float(scale), "phase")
    hit = _x3_planes.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version:
        return hit[2]
    if _capturing() or not w.is_contiguous():
        return None
    if w.dim() != 4 or tuple(w.shape[1:3]) != (3, 3) or w.shape[3] % 4:
        raise ValueError("x3_upsample_phase_planes: weight must be [Cout, 3, 3, C] with C a multiple of 4")
    lib = load()
    n, c = w.shape[0], w.shape[3]
    planes = torch.empty(2, 4, n, 4 * c, dtype=torch.float16, device=w.device)
    _check(lib.ief_x3_upsample_phase_weights(w.data_ptr(), planes.data_ptr(), n, c, float(scale), _stream()), "ief_x3_upsample_phase_weights")
    import weakref
    _x3_planes[key] = (weakref.ref(w), w._version, planes)
    weakref.finalize(w, _x3_planes.pop, key, None)
    return planes


def _x3_tiles(w, key, planes):
    """make and cache the tiled copy (`ief_x3_tile_weights`) of row-major weight planes [2, ..., K] (rows = everything between)"""
    if planes is None or _capturing():
        return None
    lib = load()
    k = planes.shape[-1]
    tiled = torch.empty_like(planes)
    _check(lib.ief_x3_tile_weights(planes.data_ptr(), tiled.data_ptr(), planes.numel() // (2 * k), k, _stream()), "ief_x3_tile_weights")
    import weakref
    _x3_planes[key] = (weakref.ref(w), w._version, tiled)
    weakref.finalize(w, _x3_planes.pop, key, None)
    return tiled


def x3_weight_tiles(w, scale=None):
    """the planes of `x3_weight_planes(w, scale)` in the TILED order the planes kernels fetch whole 128-byte lines from
    (`ief_x3_tile_weights`, IefGemmX3pParams.w_tiled): fp16 [2, N, K] holding the same halves at other addresses, a bit-copy made
    from the row-major planes at first use and cached beside them (same key plus a tag, dies with the weight).  N % 4 == 0 and
    K % 32 == 0.  None while a graph is being captured and the copy does not exist yet."""
    scale = X3_SCALE_W if scale is None else scale
    key = (w.data_ptr(), tuple(w.shape), float(scale), "tiles")
    hit = _x3_planes.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version:
        return hit[2]
    return _x3_tiles(w, key, x3_weight_planes(w, scale))


def x3_upsample_phase_tiles(w, scale=None):
    """`x3_upsample_phase_planes(w, scale)` [2, 4, Cout, 4 C] with each of the four phase matrices in the tiled order of
    `x3_weight_tiles` (Cout % 4 == 0: the four matrices of a plane tile as ONE matrix of 4 Cout rows)"""
    scale = X3_SCALE_W if scale is None else scale
    key = (w.data_ptr(), tuple(w.shape), float(scale), "phase", "tiles")
    hit = _x3_planes.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version:
        return hit[2]
    return _x3_tiles(w, key, x3_upsample_phase_planes(w, scale))


def fold_linear_pair_ref(wp, w2, b2=None, bp=None):
    """host reference of `ief_x3_fold_linear_pair` (any device, fp64 throughout): ([Wp W2 | Wp] fp64 [C, K + C], Wp b2 + bp fp64 [C])
    with (g W2^T + b2 + h) Wp^T + bp = [g | h] wcat^T + bcat"""
    wp64, w264 = wp.double(), w2.double()
    if wp64.dim() != 2 or wp64.shape[0] != wp64.shape[1] or w264.dim() != 2 or w264.shape[0] != wp64.shape[0]:
        raise ValueError("fold_linear_pair: wp must be [C, C] and w2 [C, K]")
    b = torch.zeros(wp64.shape[0], dtype=torch.float64, device=wp.device)
    if b2 is not None:
        b = wp64 @ b2.double()
    if bp is not None:
        b = b + bp.double()
    return torch.cat([wp64 @ w264, wp64], 1), b


def x3_fold_linear_pair(wp, w2, b2=None, bp=None):
    """(wcat fp32 [C, K + C], bcat fp32 [C]) of two linears folded into one (`ief_x3_fold_linear_pair`: w2 [C, K] then wp [C, C]).
    A DERIVED weight, cached per (wp, w2) pair like the phase planes: made at the first eager use (after a multi-GPU weight
    broadcast, which runs before any forward), None while a graph is being captured and it does not exist yet, re-made when either
    weight or bias was updated in place, freed with wp.  Its operand planes come from `x3_weight_planes(wcat)`."""
    key = (wp.data_ptr(), tuple(wp.shape), w2.data_ptr(), tuple(w2.shape), "fold")
    srcs = (wp, w2, b2, bp)
    hit = _x3_planes.get(key)
    if hit is not None and all((r is None and t is None) or (r is not None and r() is t and v == t._version)
                               for t, (r, v) in zip(srcs, hit[0])):
        return hit[2]
    if _capturing():
        return None
    if wp.dim() != 2 or wp.shape[0] != wp.shape[1] or w2.dim() != 2 or w2.shape[0] != wp.shape[0]:
        raise ValueError("x3_fold_linear_pair: wp must be [C, C] and w2 [C, K]")
    C, K = w2.shape
    for t, nm in ((wp, "wp"), (w2, "w2"), (b2, "b2"), (bp, "bp")):
        if t is not None and (not _dev32(t, nm).is_contiguous() or (t.dim() == 1 and t.numel() != C)):
            raise ValueError(f"x3_fold_linear_pair: {nm} must be contiguous fp32 ([C] for a bias)")
    lib = load()
    wcat = torch.empty(C, K + C, dtype=torch.float32, device=wp.device)
    bcat = torch.empty(C, dtype=torch.float32, device=wp.device)
    _check(lib.ief_x3_fold_linear_pair(wp.data_ptr(), w2.data_ptr(), _ptr(b2), _ptr(bp), wcat.data_ptr(), bcat.data_ptr(), C, K,
                                       _stream()), "ief_x3_fold_linear_pair")
    import weakref
    _x3_planes[key] = (tuple((None, 0) if t is None else (weakref.ref(t), t._version) for t in srcs), 0, (wcat, bcat))
    weakref.finalize(wp, _x3_planes.pop, key, None)
    return wcat, bcat


def _set_x3(p, sa, sb, w=None) -> str:
    """fill the split-operand fields of an IefGemmF32Params from the current mode; returns the kernel family's name.
    w: the launch's B operand when it is a weight ([N, K...] contiguous fp32): its cached pre-split planes ride along"""
    if _F32_CONTRACT == "x3":
        p.x3, p.sa, p.sb = 1, sa, sb
        if w is not None and X3_PRESPLIT and (w.numel() // w.shape[0]) % 8 == 0:
            planes = x3_weight_planes(w, sb)
            if planes is not None:
                p._planes = planes          # keep alive until the launch is queued
                p.Wp = planes.data_ptr()
        return "igemm_x3_kernel"
    return "igemm_f32_kernel"


def _is32(t) -> bool:
    """True for the fp32 activations / weights of the reference-precision mode (`csrc/exact_f32.hip`)"""
    return isinstance(t, torch.Tensor) and t.dtype == torch.float32


def _act32(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise TypeError(f"{name}: expected an fp32 device tensor (reference-precision mode), got "
                        f"{type(t).__name__ if not isinstance(t, torch.Tensor) else (t.dtype, t.device)}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: last dimension must be contiguous")
    return t


def _rows_ld_of(t, name, dev):
    """(rows, cols, ld) of a 2-D/3-D tensor whose leading dims collapse to rows with one stride; dev: the mode's tensor check"""
    dev(t, name)
    cols = t.shape[-1]
    ld = t.stride(-2) if t.dim() >= 2 else cols
    rows = 1
    for s in t.shape[:-1]:
        rows *= s
    if t.dim() == 3 and t.shape[0] > 1 and t.stride(0) != t.shape[1] * ld:
        raise ValueError(f"{name}: batch stride must equal rows * ld")
    return rows, cols, ld


def _rows_ld32(t, name):
    return _rows_ld_of(t, name, _act32)


def _dev32(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous fp32 device tensor")
    return t


def _devi32(t, name):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous int32 device tensor")
    return t


def _rows_ld(t, name):
    return _rows_ld_of(t, name, _dev16)


# ------------------------------------------------------------------------------- GEMM / conv: the launch front-end
# What the six wrappers (`gemm` / `conv3x3` on fp16 and on fp32 storage here, `planes.gemm` / `planes.conv3x3`) have in common:
# the geometry of a convolution (`conv_geometry`, shapes only) and the epilogue operands + split-K slabs of a launch
# (`_fill_epilogue`).  A wrapper keeps the check of its own tensors, its parameter struct, its plan policy and its profile record.
ConvGeometry = collections.namedtuple(
    "ConvGeometry", "B Hp Wp C1 C2 CE1 CE2 Cout H Wd Ho Wo M K rows_per_batch halo_geom phase_geom")


def _shape(t):
    return None if t is None else tuple(t.shape)


def conv_geometry(x, w, x2=None, extra=None, rowvec=None, residual=None, stride=1, upsample=False, pad_hi_only=False,
                  who="conv3x3"):
    """the geometry of one 3x3 convolution launch from SHAPES alone (tuples; `extra` = (e1, e2 | None)): x [B, Hp, Wp, C1],
    x2 [B, Hp, Wp, C2], w [Cout, 3, 3, C1 + C2] or, with extra sources [B, Ho, Wo, CE] for the fused 1x1, [Cout, K];
    rowvec [B | 1, Cout], residual [B, Ho, Wo, Cout].  (H, Wd) is the image the taps gather from (the nearest-2x of the source
    under `upsample`), M x K the implicit GEMM.  halo_geom / phase_geom: whether the geometry fits the halo form (the input
    super-tile resident in LDS across the taps) and the phase form of the fused nearest-2x (four 2x2 convolutions of the source:
    the halo form's limits on the SOURCE image) -- each mode adds its own terms.  ValueError (prefixed `who`) on a mismatch."""
    if len(x) != 4 or len(w) not in (2, 4):
        raise ValueError(f"{who}: x must be NHWC [B, H, W, C] and w [Cout, 3, 3, C] or fused [Cout, K]")
    B, Hp, Wp, C1 = x
    C2 = 0
    if x2 is not None:
        if tuple(x2[:-1]) != (B, Hp, Wp):
            raise ValueError(f"{who}: x2 spatial shape mismatch")
        C2 = x2[-1]
    H, Wd = (Hp * 2, Wp * 2) if upsample else (Hp, Wp)
    pad_total = 1 if pad_hi_only else 2
    Ho, Wo = (H + pad_total - 3) // stride + 1, (Wd + pad_total - 3) // stride + 1
    Cout = w[0]
    CE1 = CE2 = 0
    if extra is not None:
        e1, e2 = extra
        for e in (e1, e2):
            if e is not None and tuple(e[:-1]) != (B, Ho, Wo):
                raise ValueError(f"{who}: extra sources must be contiguous NHWC at the output resolution")
        CE1 = e1[-1]
        CE2 = 0 if e2 is None else e2[-1]
    M, K = B * Ho * Wo, 9 * (C1 + C2) + CE1 + CE2
    if extra is not None:
        if tuple(w) != (Cout, K):
            raise ValueError(f"{who}: fused weight must be [Cout, 9*(C1+C2)+CE1+CE2]")
    elif tuple(w[1:]) != (3, 3, C1 + C2):
        raise ValueError(f"{who}: weight shape {tuple(w)} does not match C1+C2={C1 + C2}")
    rows_per_batch = 0
    if rowvec is not None:
        if len(rowvec) != 2 or rowvec[1] != Cout or rowvec[0] not in (1, B):
            raise ValueError(f"{who}: rowvec must be [B, Cout] or [1, Cout]")
        rows_per_batch = Ho * Wo if rowvec[0] == B and B > 1 else B * Ho * Wo
    if residual is not None and tuple(residual) != (B, Ho, Wo, Cout):
        raise ValueError(f"{who}: residual must be contiguous [B, Ho, Wo, Cout]")
    plain = stride == 1 and not pad_hi_only and extra is None and Hp >= 2
    halo_geom = plain and ((not upsample and 2 <= Wd <= 64) or (upsample and Wd <= 128 and (H * Wd) % 256 == 0 and 256 % Wd == 0))
    phase_geom = plain and upsample and 2 <= Wp <= 64
    return ConvGeometry(B, Hp, Wp, C1, C2, CE1, CE2, Cout, H, Wd, Ho, Wo, M, K, rows_per_batch, bool(halo_geom), bool(phase_geom))


def _fill_epilogue(p, rows_ld, who, M, N, device, bias=None, rowvec=None, rows_per_batch=0, residual=None, splits=1):
    """the fields IefGemmParams, IefGemmF32Params and IefGemmX3pParams name alike: bias, rowvec / rows_per_batch, residual / ldr
    (rows of one stride under the mode's `_rows_ld` / `_rows_ld32`, M x N) and, for splits > 1, splits / ws.  Returns the
    split-K slabs (or None): the caller holds them until the launch is queued."""
    p.bias = _ptr(_dev32(bias, "bias")) if bias is not None else None
    if rowvec is not None:
        p.rowvec, p.rows_per_batch = _dev32(rowvec, "rowvec").data_ptr(), rows_per_batch
    if residual is not None:
        Mr, Nr, ldr = rows_ld(residual, "residual")
        if (Mr, Nr) != (M, N):
            raise ValueError(f"{who}: residual shape mismatch")
        p.residual, p.ldr = residual.data_ptr(), ldr
    if splits <= 1:
        return None
    ws = torch.empty(splits * M * N, dtype=torch.float32, device=device)
    p.splits, p.ws = splits, ws.data_ptr()
    return ws


def _conv_geometry_of(dev, x, w, x2, extra, rowvec, residual, stride, upsample, pad_hi_only):
    """`conv_geometry` of the fp16 / fp32-storage convolution after the mode's tensor check `dev` of its operands"""
    e1, e2 = (None, None) if extra is None else extra
    for t, name in ((x, "x"), (w, "w"), (x2, "x2")):
        if t is not None and not dev(t, name).is_contiguous():
            raise ValueError("conv3x3: x, x2, w must be contiguous")
    for e in (e1, e2):
        if e is not None and not dev(e, "extra").is_contiguous():
            raise ValueError("conv3x3: extra sources must be contiguous NHWC at the output resolution")
    if residual is not None and not dev(residual, "residual").is_contiguous():
        raise ValueError("conv3x3: residual must be contiguous [B, Ho, Wo, Cout]")
    return conv_geometry(x.shape, w.shape, _shape(x2), None if extra is None else (e1.shape, _shape(e2)), _shape(rowvec),
                         _shape(residual), stride, upsample, pad_hi_only)


def _conv_out(dev, out, g, dtype, device):
    if out is None:
        return torch.empty(g.B, g.Ho, g.Wo, g.Cout, dtype=dtype, device=device)
    if not dev(out, "out").is_contiguous() or out.numel() != g.M * g.Cout:
        raise ValueError("conv3x3: out must be contiguous [B, Ho, Wo, Cout]")
    return out


# ------------------------------------------------------------------------------- attention: the launch front-end
# What the attention wrappers of the three modes (here and `planes.attn_flash`) have in common: the geometry of a launch
# (`attn_geometry`, shapes only), the strided layout of an operand (`_attn_layout`) and the fields of `IefAttnF32Params` that the
# fused fp32-storage launches fill alike (`_fill_attn`).  The library sees pointers and leading dimensions only: a `v` one row
# shorter than `k` must end here, as a ValueError, not on the device as a read out of bounds.
AttnGeometry = collections.namedtuple("AttnGeometry", "B N L C d")


def attn_geometry(q, k, v, heads, out=None, do=None, o=None, lse=None, q_src=False, k_src=False, v_src=False, batch=None,
                  who="attn_flash"):
    """the geometry of one attention launch from SHAPES alone (tuples): q [Bq, N, C], k / v [Bk | Bv, L, C], C = heads * d.
    The OPERAND-BATCH rule: the launch has B = `batch` batch rows (default: q's); an operand WITHOUT a batch-row list (`q_src` /
    `k_src` / `v_src` false) must have exactly B of them, an operand WITH one may have any number -- row b of the launch reads
    batch row list[b] of it, which only the list's maker can check (`BatchRows` on the host; the lists a control plan switches
    per step live on the device), so a Bp-row q under a 2 Bp-row launch, or sources of more rows than the destination, are
    admitted.  The DESTINATION rule: `out` (the result, or the destination a gathered / class-masked launch overwrites) is
    [B, N, C] and `lse` [B, heads, N], both counted in the launch's rows; `do` / `o` (the backward's upstream gradient and forward
    output) have q's shape.  Which head dims and key counts have a kernel is not decided here (the `*_ok` predicates and the
    library's IEF_ESHAPE do that).  ValueError (prefixed `who`) on a mismatch."""
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (out, "out"), (do, "do"), (o, "o")):
        if t is not None and len(t) != 3:
            raise ValueError(f"{who}: {nm} must be [B, rows, heads*d], got {tuple(t)}")
    Bq, N, C = q
    L = k[1]
    if heads < 1 or C % heads:
        raise ValueError(f"{who}: {C} channels are not a multiple of heads = {heads}")
    if k[2] != C or v[2] != C:
        raise ValueError(f"{who}: k / v must have q's {C} channels, got {k[2]} / {v[2]}")
    if v[1] != L:
        raise ValueError(f"{who}: v must have k's {L} rows, got {v[1]}")
    if N < 1 or L < 1:
        raise ValueError(f"{who}: no queries or no keys ({N}, {L})")
    B = Bq if batch is None else int(batch)
    for t, nm, listed in ((q, "q", q_src), (k, "k", k_src), (v, "v", v_src)):
        if not listed and t[0] != B:
            raise ValueError(f"{who}: a launch of {B} batch rows over {nm} of {t[0]} needs {nm}_src")
    if out is not None and tuple(out) != (B, N, C):
        raise ValueError(f"{who}: the destination must be [{B}, {N}, {C}], got {tuple(out)}")
    for t, nm in ((do, "do"), (o, "o")):
        if t is not None and tuple(t) != (Bq, N, C):
            raise ValueError(f"{who}: {nm} must have q's shape [{Bq}, {N}, {C}], got {tuple(t)}")
    if lse is not None and tuple(lse) != (B, heads, N):
        raise ValueError(f"{who}: lse must be [B, heads, N] = [{B}, {heads}, {N}], got {tuple(lse)}")
    return AttnGeometry(B, N, L, C, C // heads)


def _attn_layout(t, name, dev):
    """(batch stride, ld) of an attention operand, gradient or destination: 3-D, unit channel stride, batch stride = rows * ld
    where there is more than one batch row (column slices of a wider projection are fine); dev: the mode's tensor check, as for
    `_rows_ld_of` (`planes._hi` for operand planes: it returns the hi plane the strides are read from)"""
    h = dev(t, name)
    if h.dim() != 3 or h.stride(2) != 1 or (h.shape[0] > 1 and h.stride(0) != h.shape[1] * h.stride(1)):
        raise ValueError(f"{name}: expected [B, rows, heads*d] with unit channel stride and batch stride rows * ld")
    return h.stride(0), h.stride(1)


def _attn_dest(t, name, dev, g):
    """a destination of the launches that carry its batch stride (IefAttnF32Params.sOb / sOPb, `_fill_attn`): [B, N, C] of the
    geometry g with unit channel stride, whose rows and batch rows do not overlap -- any batch stride from N * ld up, so o[1::2] of
    a [2 B, N, C] buffer is fine, like a column slice of a wider one.  dev: the mode's tensor check (returns what the strides are
    read from)"""
    h = dev(t, name)
    if tuple(h.shape) != (g.B, g.N, g.C):
        raise ValueError(f"{name}: the destination must be [{g.B}, {g.N}, {g.C}], got {tuple(h.shape)}")
    if h.stride(2) != 1 or h.stride(1) < g.C or (g.B > 1 and h.stride(0) < g.N * h.stride(1)):
        raise ValueError(f"{name}: expected unit channel stride, a row stride of at least {g.C} and batch rows that do not overlap")
    return h


def _attn_geometry_of(dev, who, q, k, v, heads, out=None, do=None, o=None, **kw):
    """`attn_geometry` of a launch after the mode's tensor check `dev` and the layout check of everything it is given"""
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (out, "out"), (do, "do"), (o, "o")):
        if t is not None:
            _attn_layout(t, nm, dev)
    return attn_geometry(_shape(q), _shape(k), _shape(v), heads, _shape(out), _shape(do), _shape(o), who=who, **kw)


def _grad_like(t, g, name, who):
    """the gradient buffer of operand t: fresh, or the caller's (a column slice of a wider buffer, say) of t's shape"""
    if g is None:
        return torch.empty(t.shape, dtype=t.dtype, device=t.device)
    _attn_layout(g, name, _act32 if _is32(t) else _dev16)
    if g.shape != t.shape:
        raise ValueError(f"{who}: {name} must have the shape of its operand")
    return g


def _fill_attn(p, g, heads, scale, q, k, v, q_src=None, k_src=None, v_src=None, x3=1, out=None, out_planes=False):
    """the fields of IefAttnF32Params that every fused fp32-storage attention launch fills (`_fill_epilogue`'s counterpart): the
    operands -- fp32 tensors (Q / K / V) or `planes.Planes` (Qp / Kp / Vp + plane offsets) -- with their strides, B heads N L d
    scale of the geometry g, the three batch-row lists, x3 and the destination: fresh operand planes for to_out's GEMM
    (`out_planes` true, `planes.attn_out_args`), the caller's fp32 `out`, a fresh fp32 tensor, or -- `out_planes` a Planes, what
    a gathered / class-masked launch overwrites -- the caller's planes and, if given, its fp32 `out` beside them.  The launch
    carries the destination's batch stride, so views such as o[1::2] are fine.  Operands and destination have passed
    `attn_geometry`.  Returns the result; the caller adds what is its own and launches."""
    for t, nm in ((q, "Q"), (k, "K"), (v, "V")):
        h = t
        if not isinstance(t, torch.Tensor):
            h, nm = t.hi, nm + "p"
            setattr(p, "plane" + nm[0], t.plane)
        setattr(p, nm, h.data_ptr())
        setattr(p, f"s{nm[0]}b", h.stride(0))
        setattr(p, "ld" + nm[0].lower(), h.stride(1))
    p.B, p.heads, p.N, p.L, p.d, p.scale = g.B, heads, g.N, g.L, g.d, scale
    p.q_src, p.k_src, p.v_src = _ptr(_devi32(q_src, "q_src")), _ptr(_devi32(k_src, "k_src")), _ptr(_devi32(v_src, "v_src"))
    p.x3 = x3
    dest_p = out_planes if hasattr(out_planes, "hi") else None
    if dest_p is not None:
        hp = dest_p.hi
        p.OutP, p.planeO, p.sOPb, p.ldp = hp.data_ptr(), dest_p.plane, hp.stride(0), hp.stride(1)
        if out is None:
            return dest_p
    elif out_planes:
        from . import planes as _pl
        return _pl.attn_out_args(p, g.B, g.N, g.C, h.device)[0]
    elif out is None:
        out = torch.empty(g.B, g.N, g.C, dtype=torch.float32, device=h.device)
    p.Out, p.sOb, p.ldo = _act32(out, "out").data_ptr(), out.stride(0), out.stride(1)
    return dest_p or out


def _edit_tables(mt, coef, dtype, who="attn_cross_p2p"):
    """the Prompt-to-Prompt edit tables of a launch: mt [slots, 96, 96] in the mode's dtype, coef [slots, 2, 96] fp32, contiguous,
    one coefficient pair per table (the kernels index both by edit_slot[b])"""
    if not (isinstance(mt, torch.Tensor) and mt.is_cuda and mt.dtype == dtype):
        raise TypeError(f"{who}: mt must be a {dtype} device tensor")
    _dev32(coef, "coef")
    if mt.dim() != 3 or tuple(mt.shape[1:]) != (96, 96) or not mt.is_contiguous() or tuple(coef.shape) != (mt.shape[0], 2, 96):
        raise ValueError(f"{who}: mt must be contiguous [slots,96,96] {dtype}, coef [slots,2,96] fp32 with mt's slots, got "
                         f"{tuple(mt.shape)} / {tuple(coef.shape)}")


def _edit_lists(edit_src, edit_slot, B, L, who="attn_cross_p2p"):
    """the edit pointers of a launch WITH an edit: both given, contiguous int32 device lists of exactly B entries -- the kernels
    index them by batch row and cannot check them, a short list would be read past its end -- over at most 96 keys (what the
    tables hold).  The three bindings of the edit (`_attn_cross_p2p_x3`, the fp16 launch of `attn_cross_p2p`, `p2p_cross_edit_`)
    call it before anything is launched."""
    if edit_src is None or edit_slot is None:
        raise ValueError(f"{who}: an edit needs both edit_src and edit_slot")
    for t, nm in ((edit_src, "edit_src"), (edit_slot, "edit_slot")):
        if _devi32(t, nm).dim() != 1 or t.numel() != B:
            raise ValueError(f"{who}: {nm} needs one entry per batch row ({B}), got {tuple(t.shape)}")
    if L > 96:
        raise ValueError(f"{who}: the edit tables hold 96 tokens, got {L} keys")


def gemm(a, w, bias=None, residual=None, rowvec=None, rows_per_batch=0, out=None, out_scale=1.0, tile_hint=0, splits=1,
         stages=2, geglu=False, ln=None, row_stats=False, col_stats=False, w_act=False):
    """out[..., n] = (a[..., :] . w[n, :] + bias[n] + rowvec[row // rows_per_batch, n] + residual[..., n]) * out_scale

    a: fp16 [..., K] (last dim contiguous, uniform row stride); w: fp16 [N, K]; bias/rowvec fp32.
    LayerNorm folding (see include/ief_hip.h): `row_stats=True` also returns the per-row moments of the output,
    a fp32 [M, tiles_n, 2] tensor; `ln=(stats, colsum, eps)` consumes the moments of `a`'s rows: the product is then
    rstd * (a . w - mean * colsum) + bias, i.e. LayerNorm(a) . W^T when w = W * gamma and bias carries beta . W^T.
    `col_stats=True` (a 1x1 projection over an NHWC activation): returns (out, ColStats | None) for the consuming GroupNorm.
    fp32 `a` / `w` (reference-precision mode) run on the fp32-input MFMA; LayerNorm folding does not exist there.
    `w_act=True`: w is an ACTIVATION (the keys of an attention done by GEMM), not a weight: no planes are kept of it, and in the
    split-operand mode the product runs on the fp32-input MFMA (`_gemm_f32`): no static split scale fits both operands.
    """
    if _is32(a):
        if ln is not None or row_stats:
            raise ValueError("gemm: LayerNorm folding / row statistics exist only on the fp16 path")
        if geglu and _F32_CONTRACT == "x3" and residual is None and rowvec is None and w.shape[0] % 16 == 0 and X3_FUSE_GEGLU:
            o = _gemm_f32(a, w, bias=bias, out=out, out_scale=out_scale, geglu=True)       # GEGLU in the GEMM's epilogue
            return (o, None) if col_stats else o
        o = _gemm_f32(a, w, bias=bias, residual=residual, rowvec=rowvec, rows_per_batch=rows_per_batch,
                      out=None if geglu else out, out_scale=out_scale, w_act=w_act)
        if geglu:
            o = geglu_il(o, out=out)
        return (o, None) if col_stats else o
    lib = load()
    M, K, lda = _rows_ld(a, "a")
    _dev16(w, "w")
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm: K mismatch {w.shape[1]} vs {K}")
    No_expect = N // 2 if geglu else N
    if out is None:
        out = torch.empty(*a.shape[:-1], No_expect, dtype=torch.float16, device=a.device)
    Mo, No, ldo = _rows_ld(out, "out")
    if (Mo, No) != (M, No_expect):
        raise ValueError("gemm: out shape mismatch")
    p = IefGemmParams()
    p.A, p.W, p.Out = a.data_ptr(), w.data_ptr(), out.data_ptr()
    p.M, p.N, p.K = M, N, K
    p.lda, p.ldw, p.ldo = lda, w.stride(0), ldo
    p.out_scale = out_scale
    if tile_hint == 0:
        if AUTOTUNE and f"gemm|{M}|{N}|{K}" not in _plan_table() and not _capturing() and _prof is None:
            wc = _cold_copies(w)
            autotune_plan("gemm", M, N, K, lambda t, sp, st, i: gemm(a, wc[i % len(wc)], bias=bias, residual=residual,
                                                                      rowvec=rowvec, rows_per_batch=rows_per_batch, out=out,
                                                                      out_scale=out_scale, tile_hint=t, splits=sp, stages=st,
                                                                      geglu=geglu))
            del wc
        Mp = _plan_m(M)
        p.tile_hint, p.splits, p.stages = pick_plan(Mp, N, K)
        if (geglu or ln is not None or row_stats) and p.splits > 1:
            p.tile_hint, p.splits, p.stages = heuristic_plan(Mp, N, K)[0], 1, 2
    else:
        p.tile_hint, p.splits, p.stages = tile_hint, max(1, splits), stages
    ws = _fill_epilogue(p, _rows_ld, "gemm", M, N, a.device, bias, rowvec, rows_per_batch, residual, p.splits)
    if ws is not None:
        nt, kb = _tile_count(lib, p.tile_hint, M, N, p.splits)
        p.cnt = _splitk_counters(a.device, nt, kb) if nt else None
    stats = None
    if row_stats:
        bn = lib.ief_gemm_tile_bn(p.tile_hint)
        stats = torch.empty(M, -(-N // bn), 2, dtype=torch.float32, device=a.device)
        p.rstat_out = stats.data_ptr()
    if ln is not None:
        st_in, colsum, eps = ln
        if _dev32(st_in, "ln stats").dim() != 3 or st_in.shape[0] != M or st_in.shape[2] != 2:
            raise ValueError("gemm: ln stats must be fp32 [M, slots, 2]")
        if _dev32(colsum, "colsum").numel() != N:
            raise ValueError("gemm: colsum must have N entries")
        p.rstat_in, p.rstat_slots, p.colsum, p.ln_eps = st_in.data_ptr(), st_in.shape[1], colsum.data_ptr(), eps
    p.flags, p.zeros = (3 if geglu else 1), _zeros(a.device)
    cst = None
    if col_stats and a.dim() == 4 and out.dim() == 4 and out.is_contiguous():       # a 1x1 projection over an NHWC activation
        cst = _attach_cstat(lib, p, out, M, N, a.shape[1] * a.shape[2])
    nbytes = 2.0 * (M * K + N * K + M * No_expect + (M * N if residual is not None else 0))
    with _Timed(_kname(p.tile_hint, False, p.stages) + (f" {M}x{N}x{K} s{p.splits}" if PROF_SHAPES else ""), 2.0 * M * N * K, nbytes):
        _check(lib.ief_gemm_f16(byref(p), 1, _stream()), "ief_gemm_f16")
    if col_stats:
        return out, cst
    return (out, stats) if row_stats else out


def conv3x3(x, w, bias=None, x2=None, stride=1, upsample=False, rowvec=None, residual=None, out=None, tile_hint=0,
            extra=None, splits=1, stages=2, pad_hi_only=False, col_stats=False):
    """3x3 / pad 1 convolution over NHWC fp16.  x [B,H,W,C1] (+ x2 [B,H,W,C2] channel-concat),
    w [Cout, 3, 3, C1+C2] fp16; `upsample` = nearest-2x of the input fused into the gather.
    extra=(e1, e2|None): fused 1x1 convolution over more NHWC sources sampled at the output pixel; w is
    then [Cout, 9*(C1+C2) + CE1 + CE2].  `col_stats=True`: returns (out, ColStats | None) for the consuming GroupNorm."""
    if _is32(x):
        o = _conv3x3_f32(x, w, bias, x2, stride, upsample, rowvec, residual, out, extra, pad_hi_only)
        return (o, None) if col_stats else o
    lib = load()
    g = _conv_geometry_of(_dev16, x, w, x2, extra, rowvec, residual, stride, upsample, pad_hi_only)
    B, Hp, Wp, C1, C2, CE1, CE2, Cout, H, Wd, Ho, Wo, M, K = g[:14]
    e1, e2 = (None, None) if extra is None else extra
    out = _conv_out(_dev16, out, g, torch.float16, x.device)
    p = IefGemmParams()
    p.A, p.A2, p.W, p.Out = x.data_ptr(), _ptr(x2), w.data_ptr(), out.data_ptr()
    p.N, p.ldo = Cout, Cout
    p.H, p.Wd, p.C1, p.C2 = H, Wd, C1, C2
    p.stride, p.ups, p.batch_images = stride, 1 if upsample else 0, B
    p.pad_hi_only = 1 if pad_hi_only else 0
    p.out_scale = 1.0
    if tile_hint == 0:
        variant = "|u" if upsample else ""
        if AUTOTUNE and f"conv|{M}|{Cout}|{K}{variant}" not in _plan_table() and not _capturing() and _prof is None:
            wc = _cold_copies(w)
            autotune_plan("conv", M, Cout, K, lambda t, sp, st, i: conv3x3(x, wc[i % len(wc)], bias, x2=x2, stride=stride,
                                                                            upsample=upsample, rowvec=rowvec,
                                                                            residual=residual, out=out, tile_hint=t,
                                                                            splits=sp, extra=extra, stages=st,
                                                                            pad_hi_only=pad_hi_only), variant=variant)
            del wc
        Mp = _plan_m(M)
        p.tile_hint, p.splits, p.stages = pick_plan(Mp, Cout, K, conv=True, variant=variant)
        halo_ok = g.halo_geom
        if halo_ok and HALO_HEURISTIC and f"conv|{Mp}|{Cout}|{K}{variant}" not in _plan_table() and (
                not upsample or f"conv|{Mp}|{Cout}|{K}" not in _plan_table()):
            # no measured plan for this shape: the halo kernel (256 x 80 tiles) beat the implicit GEMM on every plain 3x3
            # convolution that was tuned; cut K (whole 64-channel blocks) until ~256 workgroups exist
            tiles = -(-Mp // 256) * -(-Cout // 80)
            ncb = (C1 + C2) // 64
            sp = 1
            while tiles * sp < 192 and sp * 2 <= ncb and sp < 16:
                sp *= 2
            if tiles * sp >= 96:
                p.tile_hint, p.splits, p.stages = 15, sp, 4
        if p.tile_hint in _HALO_TILES and (not halo_ok or (upsample and p.tile_hint != 15) or p.splits > (C1 + C2) // 64):
            # the table is keyed by (M, N, K) alone: a convolution of another geometry that shares the key
            p.tile_hint, p.splits, p.stages = heuristic_plan(Mp, Cout, K) + (2,)
    else:
        p.tile_hint, p.splits, p.stages = tile_hint, max(1, splits), stages
    ws = _fill_epilogue(p, _rows_ld, "conv3x3", M, Cout, x.device, bias, rowvec, g.rows_per_batch, residual, p.splits)
    if ws is not None:
        nt, kb = _tile_count(lib, p.tile_hint, M, Cout, p.splits)
        p.cnt = _splitk_counters(x.device, nt, kb) if nt and p.tile_hint not in _HALO_TILES else None
    p.E1, p.E2, p.CE1, p.CE2 = _ptr(e1), _ptr(e2), CE1, CE2
    p.flags, p.zeros = 1, _zeros(x.device)
    cst = _attach_cstat(lib, p, out, M, Cout, Ho * Wo) if col_stats else None
    nbytes = 2.0 * (B * Hp * Wp * (C1 + C2) + M * (CE1 + CE2) + Cout * K + M * Cout * (2 if residual is not None else 1))
    with _Timed(_kname(p.tile_hint, True, p.stages) + (f" {M}x{Cout}x{K} s{p.splits}" if PROF_SHAPES else ""), 2.0 * M * Cout * K, nbytes):
        _check(lib.ief_conv3x3_f16(byref(p), _stream()), "ief_conv3x3_f16")
    return (out, cst) if col_stats else out


def _splits_f32(lib, conv, M, N, K, exact=False):
    """split-K count (1: none) for the fp32 GEMM when M x N alone gives too few 128-row tiles for the 256 CUs (the 16x16 / 8x8 levels):
    aim at ~512 workgroups, every slice keeping >= 4 K tiles of 32.  exact: the launch takes the fp32-input MFMA in either mode"""
    x3 = _F32_CONTRACT == "x3" and not exact
    nk = -(-K // 32)
    if x3:      # 128 x 80 tiles, two workgroups per CU: split below 1.5 per CU, towards 2 per CU (measured: without the split the
        # 32x32 / 16x16 levels run 1.5-2x slower than the reducer launches cost); 128 x 160 tiles, one 8-wave workgroup per CU:
        # split below one per two CUs, towards one per CU
        bn = lib.ief_gemm_x3_bn_k(1 if conv else 0, N, K)
        tiles = -(-M // lib.ief_gemm_x3_bm(M, N)) * -(-N // bn)
        below, target = (X3_SPLIT_BELOW_WIDE, X3_SPLIT_TARGET_WIDE) if bn == 160 else (X3_SPLIT_BELOW, X3_SPLIT_TARGET)
        if tiles >= below or nk < 8:
            return 1
        splits = max(1, min(-(-target // tiles), nk // 4, 16))
    else:
        tiles = -(-M // 128) * -(-N // lib.ief_gemm_f32_bn(N))
        if tiles >= 256 or nk < 8:
            return 1
        splits = max(1, min(-(-512 // tiles), nk // 4, 16))
    return splits


def _gemm_f32(a, w, bias=None, residual=None, rowvec=None, rows_per_batch=0, out=None, out_scale=1.0, transb=False, geglu=False,
              w_act=False, a_map=False):
    """fp32 out[..., n] = (a . w[n] + bias[n] + rowvec[row // rows_per_batch, n] + residual[..., n]) * out_scale;
    transb: w is [K, N] (rows along K) instead of [N, K], an activation; a_map: a is a softmax map (entries <= 1), split at
    the maps' scale; w_act: w [N, K] is an activation too (scores q k^T by GEMM).  Neither operand of that product has a
    static range: at the weights' scale a key of 256 overflowed the hi half (NaN), at the activations' scale queries of ~2^-8
    against keys of ~10^3 kept 2^-25 absolute resolution and the block missed its bound.  It runs on the fp32-input MFMA in
    both fp32-storage modes"""
    lib = load()
    M, K, lda = _rows_ld32(a, "a")
    _act32(w, "w")
    if w.dim() != 2:
        raise ValueError("gemm: w must be 2-D")
    N = w.shape[1] if transb else w.shape[0]
    if (w.shape[0] if transb else w.shape[1]) != K:
        raise ValueError(f"gemm: K mismatch {tuple(w.shape)} vs {K}")
    No_expect = N // 2 if geglu else N
    if out is None:
        out = torch.empty(*a.shape[:-1], No_expect, dtype=torch.float32, device=a.device)
    Mo, No, ldo = _rows_ld32(out, "out")
    if (Mo, No) != (M, No_expect):
        raise ValueError("gemm: out shape mismatch")
    p = IefGemmF32Params()
    p.geglu = 1 if geglu else 0
    p.A, p.W, p.Out = a.data_ptr(), w.data_ptr(), out.data_ptr()
    p.M, p.N, p.K, p.lda, p.ldw, p.ldo = M, N, K, lda, w.stride(0), ldo
    p.out_scale, p.transb = out_scale, 1 if transb else 0
    exact = w_act and not transb and not geglu
    splits = 1 if geglu else _splits_f32(lib, False, M, N, K, exact=exact)
    ws = _fill_epilogue(p, _rows_ld32, "gemm", M, N, a.device, bias, rowvec, rows_per_batch, residual, splits)     # noqa: F841  (keeps the slabs alive until the launch is queued)
    kn = "igemm_f32_kernel" if exact else _set_x3(p, X3_SCALE_PROB if a_map else X3_SCALE_ACT,
                                                  X3_SCALE_ACT if transb else X3_SCALE_W,        # transb: activation x activation
                                                  w if (not transb and w.is_contiguous()) else None)
    nbytes = 4.0 * (M * K + N * K + M * N * (2 if residual is not None else 1))
    with _Timed(f"{kn}<false, {'true' if transb else 'false'}>" + (f" {M}x{N}x{K} s{p.splits}" if PROF_SHAPES else ""), 2.0 * M * N * K, nbytes):
        _check(lib.ief_gemm_f32(byref(p), _stream()), "ief_gemm_f32")
    return out


def gemm_nt(a, b, out=None, a_map=False):
    """out = a @ b for a [M, K], b [K, N] (no transposed copy of b on the fp32 path).  `a_map=True`: a is a softmax map
    (entries <= 1); the split-operand mode then splits it at X3_SCALE_PROB as the fused attention kernels do (at scale 1
    the lo half of a probability below 2^-3 is an fp16 subnormal: at 4096 flat keys P.V was 1e-4 off, 25 x the mode's bound)"""
    if _is32(a):
        return _gemm_f32(a, b, out=out, transb=True, a_map=a_map)
    return gemm(a, transpose(b.contiguous()), out=out)


def _conv3x3_f32(x, w, bias, x2, stride, upsample, rowvec, residual, out, extra, pad_hi_only):
    lib = load()
    g = _conv_geometry_of(_act32, x, w, x2, extra, rowvec, residual, stride, upsample, pad_hi_only)
    B, Hp, Wp, C1, C2, CE1, CE2, Cout, H, Wd, Ho, Wo, M, K = g[:14]
    e1, e2 = (None, None) if extra is None else extra
    out = _conv_out(_act32, out, g, torch.float32, x.device)
    p = IefGemmF32Params()
    p.A, p.A2, p.W, p.Out = x.data_ptr(), _ptr(x2), w.data_ptr(), out.data_ptr()
    p.M, p.N, p.K, p.ldo, p.ldw = M, Cout, K, Cout, K
    p.conv, p.H, p.Wd, p.C1, p.C2, p.Ho, p.Wo = 1, H, Wd, C1, C2, Ho, Wo
    p.stride, p.ups, p.batch_images, p.pad_hi_only = stride, 1 if upsample else 0, B, 1 if pad_hi_only else 0
    p.E1, p.E2, p.CE1, p.CE2 = _ptr(e1), _ptr(e2), CE1, CE2
    p.out_scale = 1.0
    splits = _splits_f32(lib, True, M, Cout, K)
    ws = _fill_epilogue(p, _rows_ld32, "conv3x3", M, Cout, x.device, bias, rowvec, g.rows_per_batch, residual, splits)     # noqa: F841
    kn = _set_x3(p, X3_SCALE_ACT, X3_SCALE_W, w)
    nbytes = 4.0 * (B * Hp * Wp * (C1 + C2) + M * (CE1 + CE2) + Cout * K + M * Cout * (2 if residual is not None else 1))
    with _Timed(f"{kn}<true, false>" + (f" {M}x{Cout}x{K} s{p.splits}" if PROF_SHAPES else ""), 2.0 * M * Cout * K, nbytes):
        _check(lib.ief_gemm_f32(byref(p), _stream()), "ief_gemm_f32 (conv)")
    return out


def conv3x3_shortcut(h, w_fused, bias_fused, x, skip=None, col_stats=False):
    """ResnetBlock2D tail with a channel-changing shortcut in ONE launch:
    conv3x3(h) + conv1x1([x | skip]) + (b2 + bs); w_fused [Cout, 9*Cout + Cin]."""
    return conv3x3(h, w_fused, bias_fused, extra=(x, skip), col_stats=col_stats)


def softmax_rows_(x):
    """in-place softmax over the last dim of a contiguous fp16 (or, reference-precision mode, fp32) tensor"""
    lib = load()
    if _is32(x):
        if not _act32(x, "x").is_contiguous():
            raise ValueError("softmax_rows_: x must be contiguous")
        _check(lib.ief_softmax_rows_f32(x.data_ptr(), x.numel() // x.shape[-1], x.shape[-1], _stream()), "ief_softmax_rows_f32")
        return x
    _dev16(x, "x")
    if not x.is_contiguous():
        raise ValueError("softmax_rows_: x must be contiguous")
    L = x.shape[-1]
    _check(lib.ief_softmax_rows_f16(x.data_ptr(), x.numel() // L, L, _stream()), "ief_softmax_rows_f16")
    return x


def transpose(x):
    """[R, C] fp16 -> [C, R]"""
    lib = load()
    _dev16(x, "x")
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError("transpose: contiguous 2-D tensor expected")
    out = torch.empty(x.shape[1], x.shape[0], dtype=torch.float16, device=x.device)
    _check(lib.ief_transpose_f16(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _stream()), "ief_transpose_f16")
    return out


def pointwise_f32(x, w, bias=None):
    """1x1 conv on fp32 NCHW [B,Cin,H,W], w fp32 [Cout,Cin], Cin/Cout <= 8"""
    lib = load()
    _dev32(x, "x")
    _dev32(w, "w")
    B, Cin = x.shape[0], x.shape[1]
    Cout = w.shape[0]
    out = torch.empty(B, Cout, *x.shape[2:], dtype=torch.float32, device=x.device)
    _check(lib.ief_pointwise_f32(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), B, Cin, Cout,
                                 x.numel() // (B * Cin), _stream()), "ief_pointwise_f32")
    return out


def add(a, b, out=None):
    lib = load()
    if _is32(a):
        _act32(a, "a"), _act32(b, "b")
        if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
            raise ValueError("add: operands must be contiguous and of equal shape")
        out = torch.empty_like(a) if out is None else out
        _check(lib.ief_add_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "ief_add_f32")
        return out
    _dev16(a, "a")
    _dev16(b, "b")
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("add: operands must be contiguous and of equal shape")
    if out is None:
        out = torch.empty_like(a)
    _check(lib.ief_add_f16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "ief_add_f16")
    return out


def gather_rows(x, src):
    """out[b] = x[src[b]] along the batch dimension; src: device int32 [B]"""
    lib = load()
    if _is32(x):
        _devi32(src, "src")
        if not _act32(x, "x").is_contiguous() or src.numel() != x.shape[0]:
            raise ValueError("gather_rows: contiguous x [B, ...] and src [B] expected")
        out = torch.empty_like(x)
        _check(lib.ief_gather_rows_f32(x.data_ptr(), out.data_ptr(), src.data_ptr(), x.shape[0], x.numel() // x.shape[0],
                                       _stream()), "ief_gather_rows_f32")
        return out
    _dev16(x, "x")
    _devi32(src, "src")
    if not x.is_contiguous() or src.numel() != x.shape[0]:
        raise ValueError("gather_rows: contiguous x [B, ...] and src [B] expected")
    out = torch.empty_like(x)
    _check(lib.ief_gather_rows_f16(x.data_ptr(), out.data_ptr(), src.data_ptr(), x.shape[0], x.numel() // x.shape[0], _stream()),
           "ief_gather_rows_f16")
    return out


def conv_in(x, w, bias, out=None, out_planes=False):
    """latent fp32 NCHW [B,Cin,H,W] -> fp16 NHWC [B,H,W,Cout]; w fp16 [3,3,Cin,Cout] (k-major).  fp32 w: fp32 NHWC out.
    out_planes (fp32 w only): the same launch also writes the result's operand planes -> (out, planes.Planes), bit for bit
    `planes.split(out)`."""
    lib = load()
    _dev32(x, "x")
    if out_planes and not _is32(w):
        raise ValueError("conv_in: operand planes exist for the fp32-storage modes only")
    if _is32(w):
        B, Cin, H, Wd = x.shape
        if tuple(w.shape[:3]) != (3, 3, Cin) or not _act32(w, "w").is_contiguous():
            raise ValueError("conv_in: weight must be contiguous [3, 3, Cin, Cout]")
        if out is None:
            out = torch.empty(B, H, Wd, w.shape[3], dtype=torch.float32, device=x.device)
        if out_planes:
            from . import planes as _pl
            op = _pl.Planes.empty(B, H, Wd, w.shape[3], device=x.device)
            with _Timed("conv_in_f32_kernel<planes>", 2.0 * B * H * Wd * 9 * Cin * w.shape[3], 8.0 * out.numel()):
                _check(lib.ief_conv_in_f32act_planes(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), op.t.data_ptr(), op.plane,
                                                     B, Cin, H, Wd, w.shape[3], _stream()), "ief_conv_in_f32act_planes")
            return out, op
        with _Timed("conv_in_f32_kernel", 2.0 * B * H * Wd * 9 * Cin * w.shape[3], 4.0 * out.numel()):
            _check(lib.ief_conv_in_f32act(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), B, Cin, H, Wd, w.shape[3],
                                          _stream()), "ief_conv_in_f32act")
        return out
    _dev16(w, "w")
    B, Cin, H, Wd = x.shape
    if tuple(w.shape[:3]) != (3, 3, Cin) or not w.is_contiguous():
        raise ValueError("conv_in: weight must be contiguous [3, 3, Cin, Cout]")
    Cout = w.shape[3]
    if out is None:
        out = torch.empty(B, H, Wd, Cout, dtype=torch.float16, device=x.device)
    _check(lib.ief_conv_in_f32(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), B, Cin, H, Wd, Cout, _stream()),
           "ief_conv_in_f32")
    return out


def repeat_batch(*tensors):
    """every argument (a contiguous device tensor [Bp, ...] or a `planes.Planes` of such rows) repeated along the batch:
    -> tensors [2 Bp, ...] with out[r] = x[r % Bp], all written by ONE launch (`ief_repeat_batch`, up to REPEAT_MAX_JOBS
    arguments).  16-byte loads and stores: a Bp-row block whose address or size is no multiple of 16 is refused (IEF_EALIGN)."""
    lib = load()
    if not 1 <= len(tensors) <= REPEAT_MAX_JOBS:
        raise ValueError(f"repeat_batch: 1 .. {REPEAT_MAX_JOBS} tensors per launch")
    from . import planes as _pl
    jobs = (IefRepeatJob * len(tensors))()
    outs, nbytes = [], 0.0
    for j, x in zip(jobs, tensors):
        pl = isinstance(x, _pl.Planes)
        t = x.t if pl else x
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dim() >= (2 if pl else 1) and t.numel() > 0):
            raise ValueError("repeat_batch: contiguous, non-empty device tensors [Bp, ...] (or Planes of them) expected")
        blocks = 2 if pl else 1
        shape = list(t.shape)
        shape[1 if pl else 0] *= 2
        o = torch.empty(shape, dtype=t.dtype, device=t.device)
        j.src, j.dst, j.bytes, j.blocks = t.data_ptr(), o.data_ptr(), t.numel() * t.element_size() // blocks, blocks
        nbytes += 3.0 * t.numel() * t.element_size()
        outs.append(_pl.Planes(o) if pl else o)
    with _Timed("repeat_batch_kernel", 0.0, nbytes):
        _check(lib.ief_repeat_batch(jobs, len(tensors), _stream()), "ief_repeat_batch")
    return outs[0] if len(outs) == 1 else tuple(outs)


def conv_out(x, w, bias, out=None):
    """fp16 NHWC [B,H,W,C] -> fp32 NCHW [B,Cout,H,W]; w fp16 [Cout,3,3,C] (both fp32 in the reference-precision mode)."""
    lib = load()
    if _is32(x):
        B, H, Wd, C = x.shape
        if not _act32(x, "x").is_contiguous() or not _act32(w, "w").is_contiguous() or tuple(w.shape[1:]) != (3, 3, C):
            raise ValueError("conv_out: contiguous NHWC x and [Cout, 3, 3, C] weight expected")
        if out is None:
            out = torch.empty(B, w.shape[0], H, Wd, dtype=torch.float32, device=x.device)
        _check(lib.ief_conv_out_f32act(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), B, C, H, Wd, w.shape[0],
                                       _stream()), "ief_conv_out_f32act")
        return out
    _dev16(x, "x")
    _dev16(w, "w")
    B, H, Wd, C = x.shape
    Cout = w.shape[0]
    if out is None:
        out = torch.empty(B, Cout, H, Wd, dtype=torch.float32, device=x.device)
    _check(lib.ief_conv_out_f32(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), B, C, H, Wd, Cout, _stream()),
           "ief_conv_out_f32")
    return out


# ------------------------------------------------------------------------------- norms
def groupnorm(x, gamma, beta, groups, eps, silu=False, x2=None, out=None, return_stats=False, cstat=None, cstat2=None):
    """GroupNorm over NHWC / tokens-major fp16 [B, ..., C] (+ optional channel-concat x2), optional SiLU.
    return_stats: also return the fp32 (mean, rstd) [B, groups, 2] the backward reuses.
    cstat / cstat2: the ColStats the launches that PRODUCED x / x2 returned (`col_stats=True`), or None."""
    lib = load()
    if _is32(x):
        if return_stats:        # the fp32 backward recomputes its (two-pass) statistics: nothing to hand over
            return groupnorm(x, gamma, beta, groups, eps, silu=silu, x2=x2, out=out), None
        if not _act32(x, "x").is_contiguous() or (x2 is not None and not _act32(x2, "x2").is_contiguous()):
            raise ValueError("groupnorm: inputs must be contiguous")
        B, C1 = x.shape[0], x.shape[-1]
        C2 = 0 if x2 is None else x2.shape[-1]
        HW = x.numel() // (B * C1)
        if out is None:
            out = torch.empty(*x.shape[:-1], C1 + C2, dtype=torch.float32, device=x.device)
        if GN3_F32 and C1 % 4 == 0 and C2 % 4 == 0:
            nws = lib.ief_groupnorm_f32_ws_floats(B, HW, C1 + C2)
            ws = torch.empty(nws, dtype=torch.float32, device=x.device)
            with _Timed("gn3_f32 (stats + finalize + apply)", 0.0, 12.0 * (x.numel() + (0 if x2 is None else x2.numel()))):
                _check(lib.ief_groupnorm_silu_f32_ws(x.data_ptr(), _ptr(x2), C1, C2, out.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                                     _dev32(beta, "beta").data_ptr(), B, HW, groups, eps, 1 if silu else 0,
                                                     ws.data_ptr(), nws, _stream()), "ief_groupnorm_silu_f32_ws")
            return out
        with _Timed("groupnorm_f32_kernel", 0.0, 8.0 * (x.numel() + (0 if x2 is None else x2.numel()))):
            _check(lib.ief_groupnorm_silu_f32(x.data_ptr(), _ptr(x2), C1, C2, out.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                              _dev32(beta, "beta").data_ptr(), B, HW, groups, eps, 1 if silu else 0, _stream()),
                   "ief_groupnorm_silu_f32")
        return out
    _dev16(x, "x")
    if not x.is_contiguous() or (x2 is not None and not x2.is_contiguous()):
        raise ValueError("groupnorm: inputs must be contiguous")
    B, C1 = x.shape[0], x.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    HW = x.numel() // (B * C1)
    if out is None:
        out = torch.empty(*x.shape[:-1], C1 + C2, dtype=torch.float16, device=x.device)
    cs1, cs2 = cstat, None if x2 is None else cstat2
    for t, c, nm in ((x, cs1, "cstat"), (x2, cs2, "cstat2")):
        if c is not None and not c.describes(t):
            raise ValueError(f"groupnorm: {nm} was produced for another tensor (address / size mismatch)")
    if (GN_CSTAT and not return_stats and cs1 is not None and cs1.hw == HW
            and (x2 is None or (cs2 is not None and cs2.hw == HW))):
        # statistics were left by the producers' epilogues: fold them and apply — ONE launch while the fold is small
        # (2-8 tiles per image: the 32x32 / 16x16 levels), a fold launch + an apply launch above
        stats = torch.empty(B * groups * 2, dtype=torch.float32, device=x.device)
        with _Timed("groupnorm(stats+apply)", 0.0, 4.0 * x.numel() + (0 if x2 is None else 4.0 * x2.numel())):
            _check(lib.ief_groupnorm_cstat_f16(x.data_ptr(), _ptr(x2), C1, C2, out.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                               _dev32(beta, "beta").data_ptr(), cs1.buf.data_ptr(), cs1.bm,
                                               None if cs2 is None else cs2.buf.data_ptr(), 0 if cs2 is None else cs2.bm,
                                               stats.data_ptr(), B, HW, groups, eps, 1 if silu else 0, _stream()),
                   "ief_groupnorm_cstat_f16")
        return out
    splits = lib.ief_gn_splits(HW)
    partial = torch.empty(B * (splits + 1) * groups * 2, dtype=torch.float32, device=x.device)
    with _Timed("groupnorm(stats+apply)", 0.0, 4.0 * x.numel() + (0 if x2 is None else 4.0 * x2.numel())):
        _check(lib.ief_groupnorm_silu_f16(x.data_ptr(), _ptr(x2), C1, C2, out.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                          _dev32(beta, "beta").data_ptr(), partial.data_ptr(), B, HW, groups, eps,
                                          1 if silu else 0, _stream()), "ief_groupnorm_silu_f16")
    if return_stats:
        return out, partial[B * splits * groups * 2:].view(B, groups, 2)
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    lib = load()
    if _is32(x):
        if not _act32(x, "x").is_contiguous():
            raise ValueError("layernorm: x must be contiguous")
        out = torch.empty_like(x) if out is None else out
        _check(lib.ief_layernorm_f32(x.data_ptr(), out.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                     _dev32(beta, "beta").data_ptr(), x.numel() // x.shape[-1], x.shape[-1], eps, _stream()),
               "ief_layernorm_f32")
        return out
    _dev16(x, "x")
    if not x.is_contiguous():
        raise ValueError("layernorm: x must be contiguous")
    C = x.shape[-1]
    rows = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    _check(lib.ief_layernorm_f16(x.data_ptr(), out.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                 _dev32(beta, "beta").data_ptr(), rows, C, eps, _stream()), "ief_layernorm_f16")
    return out


def geglu(x, out=None):
    lib = load()
    _dev16(x, "x")
    if not x.is_contiguous():
        raise ValueError("geglu: x must be contiguous")
    Ch = x.shape[-1] // 2
    rows = x.numel() // (2 * Ch)
    if out is None:
        out = torch.empty(*x.shape[:-1], Ch, dtype=torch.float16, device=x.device)
    _check(lib.ief_geglu_f16(x.data_ptr(), out.data_ptr(), rows, Ch, _stream()), "ief_geglu_f16")
    return out


# ------------------------------------------------------------------------------- attention
def _attn_common(p, who, q, k, v, out, heads, **kw):
    """the operands of an fp16 attention launch (IefAttnParams / IefCrossParams / IefAttnBwdParams name them alike) after
    `attn_geometry`; kw: its lse / *_src / do / o"""
    g = _attn_geometry_of(_dev16, who, q, k, v, heads, out, **kw)
    p.Q, p.K, p.V = q.data_ptr(), k.data_ptr(), v.data_ptr()
    p.B, p.heads, p.N, p.L, p.d = g.B, heads, g.N, g.L, g.d
    p.ldq, p.ldk, p.ldv = q.stride(1), k.stride(1), v.stride(1)
    if out is not None:
        p.Out, p.ldo = out.data_ptr(), out.stride(1)
    return g


_FLASH_VARIANT_ENV = int(os.environ.get("IEF_FLASH_VARIANT", "0"))      # read once: which flash kernel variant 0 means


def _batched32(t, d, which):
    """strides of a [B, rows, heads*d] fp32 operand of a batched product: per batch row, per head and per row"""
    sb, ld = _attn_layout(t, which, _act32)
    return sb, d, ld


X3_SPLIT_BELOW = int(os.environ.get("IEF_X3_SPLIT_BELOW", "384"))      # split-K policy of the x3 GEMM (A/B runs)
X3_SPLIT_TARGET = int(os.environ.get("IEF_X3_SPLIT_TARGET", "512"))
X3_SPLIT_BELOW_WIDE = int(os.environ.get("IEF_X3_SPLIT_BELOW_WIDE", "129"))
X3_SPLIT_TARGET_WIDE = int(os.environ.get("IEF_X3_SPLIT_TARGET_WIDE", "256"))
GN3_F32 = os.environ.get("IEF_GN3_F32", "1") == "1"          # 0: the one-launch fp32 GroupNorm (A/B runs)
FLASH_F32 = os.environ.get("IEF_FLASH_F32", "1") == "1"      # 0: always materialise the fp32 maps (A/B runs)
X3_FUSE_CROSS = os.environ.get("IEF_X3_FUSE_CROSS", "1") == "1"      # 0: materialised cross maps (scores, softmax, edit, apply: A/B runs)
X3_FUSED_BWD = os.environ.get("IEF_X3_FUSED_BWD", "1") == "1"      # 0: the reverse pass keeps the materialised maps everywhere (A/B runs)


# ------------------------------------------------------------------------------- attention: which kernel takes a layer
# Pure host predicates of (head dim, key count, mode, switches); every set of head dims is written once, here (the operand-planes
# kernel's is `planes.FLASH_PLANES_DIMS`).  The library refuses what they do not admit (IEF_ESHAPE).
_FLASH_F32_DIMS = (32, 40, 64, 80, 160)         # attn_flash_f32_kernel / attn_flash_x3_kernel (`ief_attn_flash_f32` on fp32 operands)
_CROSS_P2P_X3_DIMS = (40, 64, 80, 160)
CROSS_MAP_GRAD_MAX_L = cabi.defines["IEF_CROSS_MAP_GRAD_MAX_L"]
_CROSS_MAP_GRAD_DIMS = (32, 40, 64, 80, 160)
CROSS_BWD_MAX_L = cabi.defines["IEF_CROSS_BWD_MAX_L"]
_CROSS_BWD_ROUTED_DIMS = (32, 40, 64, 80)


def cross_p2p_x3_ok(d, L) -> bool:
    """`attn_cross_p2p_x3_kernel` (the edited cross-attention of the f16x3 mode in one launch) has this shape: the edit tables
    hold 96 tokens.  The mode and the IEF_X3_FUSE_CROSS / IEF_FLASH_F32 switches are the caller's terms."""
    return int(d) in _CROSS_P2P_X3_DIMS and int(L) <= 96


def x3_fused_bwd_ok(d: int, L: int) -> bool:
    """the fp32-storage reverse pass differentiates this attention layer with `ief_attn_bwd_x3` (P and dS recomputed per tile from
    the forward's lse, no map in HBM): split-operand mode, head dims 40 / 64 (the levels whose maps are hundreds of MB), at
    least 128 keys (self-attention; the 77-key cross maps are small and keep the materialised path)"""
    return X3_FUSED_BWD and _F32_CONTRACT == "x3" and FLASH_F32 and d in (40, 64) and L >= 128


def cross_map_grad_ok(d, L, dtype=torch.float32) -> bool:
    """`cross_map_grad` takes this cross-attention module: fp32 operands, a head dim of the kernel's set and at most
    CROSS_MAP_GRAD_MAX_L keys (the LDS image of K, V and the two per-query columns fits a CU).  Everything else keeps
    `attn_bwd(want_dkv=False)` + `attn_map_loss_bwd`."""
    return dtype == torch.float32 and int(d) in _CROSS_MAP_GRAD_DIMS and 1 <= int(L) <= CROSS_MAP_GRAD_MAX_L


def cross_bwd_ok(d, L, dtype=torch.float32) -> bool:
    """the reverse pass differentiates this attention with `cross_bwd`: fp32 operands, at most CROSS_BWD_MAX_L keys (the LDS image
    of K, V, the two per-query columns and a workgroup's q / dO rows fits a CU) and a head dim of 32 / 40 / 64 / 80 -- a shape rule,
    no switch.  The kernel also takes d = 160, but that head dim belongs to the 16 x 16 and 8 x 8 levels, whose few workgroups sit on
    the kernel's latency floor: measured 63-76 us per module against 50-72 us materialised, so those levels,
    like everything else, keep the materialised maps of `_attn_bwd_f32`."""
    return dtype == torch.float32 and int(d) in _CROSS_BWD_ROUTED_DIMS and 1 <= int(L) <= CROSS_BWD_MAX_L


def _attn_flash_f32(q, k, v, heads, scale, q_src=None, k_src=None, v_src=None, out=None, out_planes=False, lse=None, key_splits=1,
                    batch=None):
    """fused fp32 attention (`ief_attn_flash_f32`): no map is written; None when the head dim has no instantiation.
    batch: the launch's batch rows where q has fewer of them and q_src (checked by the caller) selects among them
    out_planes (split-operand mode only): the result leaves as operand planes for to_out's GEMM (`planes.Planes`);
    lse (split-operand mode only): fp32 [B, heads, N] receiving the row log-sum-exp (log2 units) for `ief_attn_bwd_x3`"""
    lib = load()
    g = _attn_geometry_of(_act32, "attn_flash", q, k, v, heads, None if out_planes else out, lse=_shape(lse), batch=batch,
                          q_src=q_src is not None, k_src=k_src is not None, v_src=v_src is not None)
    B, N, L, d = g.B, g.N, g.L, g.d
    if not FLASH_F32 or d not in _FLASH_F32_DIMS:
        return None
    if out_planes and _F32_CONTRACT != "x3":
        raise ValueError("attn_flash: operand planes exist in the split-operand mode only")
    p = IefAttnF32Params()
    res = _fill_attn(p, g, heads, scale, q, k, v, q_src, k_src, v_src, 1 if _F32_CONTRACT == "x3" else 0, out, out_planes)
    if lse is not None:
        if not p.x3:
            raise ValueError("attn_flash: lse (contiguous fp32 [B, heads, N]) is written by the split-operand kernel only")
        p.lse = _dev32(lse, "lse").data_ptr()
    p.key_splits = int(key_splits)      # > 1: the library refuses (IEF_EINVAL) -- only the operand-planes kernel splits its keys
    with _Timed(f"attn_flash_{'x3' if p.x3 else 'f32'}_kernel<{d}>", 4.0 * B * heads * N * L * d, 4.0 * B * heads * d * (2 * N + 2 * L)):
        _check(lib.ief_attn_flash_f32(byref(p), _stream()), "ief_attn_flash_f32")
    return res


def _attn_scores_f32(q, k, heads, scale, q_src=None, k_src=None, out=None, softmax=True):
    """materialised maps softmax(scale q k^T) as contiguous fp32 [B*heads, N, L] (`register.py:43-47`): one batched
    launch of the fp32 GEMM over (batch row, head) + a row softmax (softmax=False: the scaled scores themselves)"""
    lib = load()
    _act32(q, "q"), _act32(k, "k")
    B, N, C = q.shape
    L = k.shape[1]
    d = C // heads
    if out is None:
        out = torch.empty(B * heads, N, L, dtype=torch.float32, device=q.device)
    elif tuple(_act32(out, "out").shape) != (B * heads, N, L) or not out.is_contiguous():
        raise ValueError("attn_probs: out must be contiguous fp32 [B*heads, N, L]")
    p = IefGemmF32Params()
    p.A, p.W, p.Out = q.data_ptr(), k.data_ptr(), out.data_ptr()
    p.M, p.N, p.K = N, L, d
    p.sAb, p.sAh, p.lda = _batched32(q, d, "q")
    p.sWb, p.sWh, p.ldw = _batched32(k, d, "k")
    p.sOb, p.sOh, p.ldo = heads * N * L, N * L, L
    p.batch, p.heads, p.out_scale = B, heads, scale
    p.a_src, p.w_src = _ptr(_devi32(q_src, "q_src")), _ptr(_devi32(k_src, "k_src"))
    kn = _set_x3(p, X3_SCALE_ACT, X3_SCALE_ACT)
    with _Timed(f"{kn}<scores {d}>", 2.0 * B * heads * N * L * d, 4.0 * B * heads * (N * d + L * d + N * L)):
        _check(lib.ief_gemm_f32(byref(p), _stream()), "ief_gemm_f32 (attention scores)")
    if softmax:
        with _Timed("softmax_rows_f32_kernel", 0.0, 8.0 * out.numel()):
            _check(lib.ief_softmax_rows_f32(out.data_ptr(), out.numel() // L, L, _stream()), "ief_softmax_rows_f32")
    return out


def attn_scores(q, k, heads, scale):
    """-> (sim, attn): the PRE-softmax scores scale * q k^T and their row softmax, both contiguous [B*heads, N, L] in q's
    dtype — the two tensors MasaCtrl's editor protocol hands to user editors
    (`/root/reference/masactrl/model/register.py:35,44`).  Generic-path only: computed on the fp32 MFMA / fp32 softmax
    whatever the model's storage dtype (any key count, e.g. 77)."""
    half = not _is32(q)
    if half:
        q, k = to_f32(_dev16(q, "q")), to_f32(_dev16(k, "k"))
    sim = _attn_scores_f32(q, k, heads, scale, softmax=False)
    probs = softmax_rows_(sim.clone())
    return (to_f16(sim), to_f16(probs)) if half else (sim, probs)


def _attn_apply_f32(probs, v, heads, v_src=None, out=None, map_scale=None):
    """out [B, N, heads*d] = probs [B*heads, N, L] @ v [B, L, heads*d] per (batch row, head), fp32.
    map_scale: split scale of the maps (default 2^14: entries <= 1; edited maps can exceed 1, `map_split_scale`)"""
    lib = load()
    _act32(probs, "probs"), _act32(v, "v")
    if not probs.is_contiguous():
        raise ValueError("attn_apply: probs must be contiguous")
    B = v.shape[0]
    N, L = probs.shape[1], probs.shape[2]
    d = v.shape[2] // heads
    if probs.shape[0] != B * heads or v.shape[1] != L:
        raise ValueError("attn_apply: shape mismatch")
    if out is None:
        out = torch.empty(B, N, v.shape[2], dtype=torch.float32, device=v.device)
    p = IefGemmF32Params()
    p.A, p.W, p.Out = probs.data_ptr(), v.data_ptr(), out.data_ptr()
    p.M, p.N, p.K = N, d, L
    p.sAb, p.sAh, p.lda = heads * N * L, N * L, L
    p.sWb, p.sWh, p.ldw = _batched32(v, d, "v")
    p.sOb, p.sOh, p.ldo = _batched32(out, d, "out")
    p.batch, p.heads, p.out_scale, p.transb = B, heads, 1.0, 1
    p.w_src = _ptr(_devi32(v_src, "v_src"))
    kn = _set_x3(p, X3_SCALE_PROB if map_scale is None else map_scale, X3_SCALE_ACT)    # maps <= 1: a large scale keeps the lo halves of small entries normal
    with _Timed(f"{kn}<apply {d}>", 2.0 * B * heads * N * L * d, 4.0 * B * heads * (N * d + L * d + N * L)):
        _check(lib.ief_gemm_f32(byref(p), _stream()), "ief_gemm_f32 (attention apply)")
    return out


def p2p_cross_edit_(probs, B, heads, edit_src, edit_slot, mt32, coef):
    """in place on fp32 maps [B*heads, N, L]: P'[w] = c1[w] (P_src M)[w] + c2[w] P_tgt[w] for the rows edit_src marks.  P_src is
    always the UNEDITED map of the source row: a source row that this launch edits too (from another row) is set aside first, by
    a launch that copies nothing where no such row exists (the scratch is handed over untouched then)"""
    lib = load()
    _edit_tables(mt32, coef, torch.float32, "p2p_cross_edit_")
    if not _act32(probs, "probs").is_contiguous():
        raise ValueError("p2p_cross_edit_: probs must be contiguous")
    if probs.dim() != 3 or probs.shape[0] != B * heads:
        raise ValueError(f"p2p_cross_edit_: probs must be [B*heads, N, L] = [{B * heads}, N, L], got {tuple(probs.shape)}")
    _edit_lists(edit_src, edit_slot, B, probs.shape[2], "p2p_cross_edit_")
    keep = torch.empty_like(probs)
    _check(lib.ief_p2p_cross_edit_keep_f32(probs.data_ptr(), keep.data_ptr(), edit_src.data_ptr(), edit_slot.data_ptr(),
                                           mt32.data_ptr(), coef.data_ptr(), B, heads, probs.shape[1], probs.shape[2], _stream()),
           "ief_p2p_cross_edit_keep_f32")
    return probs


def attn_flash(q, k, v, heads, scale, q_src=None, k_src=None, v_src=None, out=None, lse=None, variant=0, out_planes=False,
               key_splits=1):
    """out[b] = softmax(q[q_src[b]] k[k_src[b]]^T * scale) v[v_src[b]]; q [B,N,h*d], k/v [B,L,h*d] (strided views ok).
    lse: optional fp32 [B, heads, N] receiving the row log-sum-exp (log2 units) that `attn_bwd` consumes.
    fp32 operands (reference-precision mode): the maps are materialised in HBM, as the reference does.
    key_splits: the keys over several workgroups exists for operand planes only (`planes.attn_flash`); > 1 here is refused."""
    if key_splits != 1 and not (_is32(q) and FLASH_F32):
        raise ValueError("attn_flash: key_splits exists on operand planes only (planes.attn_flash)")
    if _is32(q):
        if lse is not None and not x3_fused_bwd_ok(q.shape[2] // heads, k.shape[1]):
            raise ValueError("attn_flash: on fp32 operands lse exists only where ief_attn_bwd_x3 consumes it (x3_fused_bwd_ok); "
                             "elsewhere the fp32 backward recomputes the maps")
        o = _attn_flash_f32(q, k, v, heads, scale, q_src, k_src, v_src, out, out_planes=out_planes, lse=lse, key_splits=key_splits)
        if o is not None:
            return o
        if lse is not None:
            raise ValueError("attn_flash: the fused fp32 kernel is switched off (IEF_FLASH_F32=0): no lse")
        o = _attn_apply_f32(_attn_scores_f32(q, k, heads, scale, q_src, k_src), v, heads, v_src, out)
        if out_planes:
            from . import planes as _pl
            return _pl.split(o)
        return o
    lib = load()
    if out is None:
        out = torch.empty(q.shape[0], q.shape[1], q.shape[2], dtype=torch.float16, device=q.device)
    p = IefAttnParams()
    _attn_common(p, "attn_flash", q, k, v, out, heads, lse=_shape(lse), q_src=q_src is not None, k_src=k_src is not None,
                 v_src=v_src is not None)
    p.scale = scale
    p.variant = variant if variant else _FLASH_VARIANT_ENV                              # env: A/B runs only
    if lse is not None:
        p.lse = _dev32(lse, "lse").data_ptr()
    p.q_src, p.k_src, p.v_src = _ptr(_devi32(q_src, "q_src")), _ptr(_devi32(k_src, "k_src")), _ptr(_devi32(v_src, "v_src"))
    kern = {1: "attn_flash_kernel", 2: "attn_flash_pp_kernel"}.get(p.variant, "attn_flash_sp_kernel")
    with _Timed(f"{kern}<{p.d}>", 4.0 * p.B * p.heads * p.N * p.L * p.d, 2.0 * p.B * p.heads * p.d * (2 * p.N + 2 * p.L)):
        _check(lib.ief_attn_flash_f16(byref(p), _stream()), "ief_attn_flash_f16")
    return out


def map_split_scale(coef_bound: float) -> float:
    """power-of-two scale for the hi / lo split of EDITED maps P' = c1 T + c2 P whose entries reach `coef_bound` = max_w (|c1| +
    |c2|) (maps <= 1 otherwise): the largest 2^k <= 2^14 with 2^k * coef_bound inside the fp16 range.  AttentionReweight lowers to
    c1 = alpha * equalizer (`/root/reference/p2p/model/attention_control.py:42-46`): with the fixed 2^14 an equalizer of 5 on a
    peaky source map overflowed to inf / NaN"""
    b = max(1.0, float(coef_bound))
    s = X3_SCALE_PROB
    while s > 1.0 and s * b > 32768.0:        # a factor 2 of head-room below 65504
        s *= 0.5
    return s


class BatchRows:
    """a batch-row indirection list built ON THE HOST and checked there: `dev` int32 [B] on the device, every entry a row of an
    operand with `rows` batch rows.  The kernels cannot check device lists; the lists a control plan switches per step live on the
    device only, this one is fixed for the life of its loop, so the check happens where it is built."""
    __slots__ = ("dev", "rows", "n")

    def __init__(self, entries, rows, device):
        entries = [int(e) for e in entries]
        if not entries or any(e < 0 or e >= rows for e in entries):
            raise ValueError(f"batch-row list {entries}: every entry must be a row of an operand with {rows} batch rows")
        self.rows, self.n = int(rows), len(entries)
        self.dev = torch.tensor(entries, dtype=torch.int32, device=device)


_cfg_rows = {}


def cfg_q_rows(Bp, device):
    """q_src of a launch over a CFG batch of 2 Bp rows whose halves share ONE Bp-row query projection: [0..Bp-1, 0..Bp-1].
    One list per (Bp, device), made at the first eager use (a captured graph keeps reading it; none is made while capturing)."""
    key = (int(Bp), str(torch.device(device)))
    r = _cfg_rows.get(key)
    if r is None:
        if _capturing():
            raise RuntimeError("cfg_q_rows: run one eager forward of this batch before capturing")
        r = _cfg_rows[key] = BatchRows(list(range(Bp)) * 2, Bp, device)
    return r


def _cfg_rows_of(q_src, q, k):
    """the device list of a cross-attention launch's q_src: a `BatchRows` built for q's batch rows, one entry per batch row of k"""
    if not isinstance(q_src, BatchRows) or q_src.rows != q.shape[0] or q_src.n != k.shape[0]:
        raise ValueError("attn_cross_p2p: q_src must be a hip.BatchRows with one entry per batch row of k / v, checked against "
                         "the batch rows of q")
    return q_src.dev


def _attn_cross_p2p_x3(q, k, v, heads, scale, edit_src, edit_slot, mt32, coef, out=None, out_planes=False, coef_bound=1.0,
                       q_src=None):
    """`ief_attn_cross_p2p_f32`: the edited cross-attention layer of the f16x3 mode in one launch (maps stay in registers).
    coef_bound: max_w (|c1| + |c2|) over the plan's coefficient tables (sizes the split of the edited maps).
    edit_src None: plain attention by the same kernel.  q_src (`BatchRows`): the launch's batch is k's; row b reads q[q_src[b]].
    out: the caller's fp32 destination (`_attn_dest`: o[1::2] of a wider batch, a column slice); out_planes True: fresh operand
    planes instead (out is then not used), a `planes.Planes` destination: the caller's planes, and with out= both from one launch."""
    lib = load()
    rows = None if q_src is None else _cfg_rows_of(q_src, q, k)
    g = _attn_geometry_of(_act32, "attn_cross_p2p", q, k, v, heads, q_src=q_src is not None,
                          batch=None if q_src is None else k.shape[0])
    B, N, L, d = g.B, g.N, g.L, g.d
    if not cross_p2p_x3_ok(d, L):
        raise ValueError(f"attn_cross_p2p: attn_cross_p2p_x3_kernel has head dims 40 / 64 / 80 / 160 and at most 96 keys, got {d} / {L}")
    if hasattr(out_planes, "hi"):
        _attn_dest(out_planes, "out_planes", lambda t, nm: _dev16(t.hi, nm), g)
    if out is not None and (not out_planes or hasattr(out_planes, "hi")):
        _attn_dest(out, "out", _act32, g)
    if edit_src is not None:
        _edit_tables(mt32, coef, torch.float32)
        _edit_lists(edit_src, edit_slot, B, L)
    p = IefAttnF32Params()
    res = _fill_attn(p, g, heads, scale, q, k, v, q_src=rows, out=out, out_planes=out_planes)
    p.p_scale = map_split_scale(coef_bound)
    nedit = 2.0 * B * heads * N * 96 * 96 if edit_src is not None else 0.0
    with _Timed(f"attn_cross_p2p_x3_kernel<{d}>", 4.0 * B * heads * N * L * d + nedit, 4.0 * B * heads * d * (2 * N + 2 * L)):
        _check(lib.ief_attn_cross_p2p_f32(byref(p), _ptr(edit_src), _ptr(edit_slot), _ptr(mt32) if edit_src is not None else None,
                                          _ptr(coef) if edit_src is not None else None, _stream()), "ief_attn_cross_p2p_f32")
    return res


def attn_cross_p2p(q, k, v, heads, scale, edit_src=None, edit_slot=None, mt=None, coef=None, out=None, out_planes=False,
                   coef_bound=1.0, q_src=None):
    """Cross-attention (<= 96 keys) with the fused Prompt-to-Prompt map edit (see include/ief_hip.h).
    fp32 operands: materialised maps, `mt` must then be the fp32 table.  out_planes (split-operand mode): the result as operand
    planes for to_out's GEMM; coef_bound: max (|c1| + |c2|) of the plan (sizes the split of the edited maps).
    q_src (`BatchRows`, split-operand mode, L <= 96 only): k / v carry the launch's batch rows, row b reads q[q_src[b]] -- the edited
    layer on `attn_cross_p2p_x3_kernel`, the unedited one on the flash kernel it takes anyway; no other route (ValueError)."""
    if q_src is not None:
        if not (_is32(q) and _F32_CONTRACT == "x3" and cross_p2p_x3_ok(q.shape[2] // heads, k.shape[1])):
            raise ValueError("attn_cross_p2p: q_src exists on the fused split-operand kernel only (f16x3, <= 96 keys, head dim 40 / "
                             "64 / 80 / 160)")
        if edit_src is None and FLASH_F32:      # the launch the unedited layer takes without q_src, hence its bits
            return _attn_flash_f32(q, k, v, heads, scale, q_src=_cfg_rows_of(q_src, q, k), out=out, out_planes=out_planes,
                                   batch=k.shape[0])
        return _attn_cross_p2p_x3(q, k, v, heads, scale, edit_src, edit_slot, mt, coef, out, out_planes, coef_bound, q_src=q_src)
    if _is32(q):
        if edit_src is None:
            o = _attn_flash_f32(q, k, v, heads, scale, out=out, out_planes=out_planes)
            if o is not None:
                return o
        elif _F32_CONTRACT == "x3" and X3_FUSE_CROSS and cross_p2p_x3_ok(q.shape[2] // heads, k.shape[1]):
            return _attn_cross_p2p_x3(q, k, v, heads, scale, edit_src, edit_slot, mt, coef, out, out_planes, coef_bound)
        g = _attn_geometry_of(_act32, "attn_cross_p2p", q, k, v, heads, out)
        if edit_src is not None:                # refused before the scores are launched, not between two of the four launches
            _edit_tables(mt, coef, torch.float32)
            _edit_lists(edit_src, edit_slot, g.B, g.L)
        probs = _attn_scores_f32(q, k, heads, scale)
        if edit_src is not None:
            p2p_cross_edit_(probs, q.shape[0], heads, edit_src, edit_slot, mt, coef)
        o = _attn_apply_f32(probs, v, heads, None, out, map_scale=map_split_scale(coef_bound) if edit_src is not None else None)
        if out_planes:
            from . import planes as _pl
            return _pl.split(o)
        return o
    lib = load()
    if out is None:
        out = torch.empty(q.shape[0], q.shape[1], q.shape[2], dtype=torch.float16, device=q.device)
    p = IefCrossParams()
    g = _attn_common(p, "attn_cross_p2p", q, k, v, out, heads)
    p.scale = scale
    if edit_src is not None:
        _edit_tables(mt, coef, torch.float16)
        _edit_lists(edit_src, edit_slot, g.B, g.L)
        p.edit_src, p.edit_slot, p.MT, p.coef = edit_src.data_ptr(), edit_slot.data_ptr(), mt.data_ptr(), coef.data_ptr()
    with _Timed(f"attn_cross_p2p_kernel<{p.d}>", 4.0 * p.B * p.heads * p.N * p.L * p.d,
                2.0 * p.B * p.heads * p.d * (2 * p.N + 2 * p.L)):
        _check(lib.ief_attn_cross_p2p_f16(byref(p), _stream()), "ief_attn_cross_p2p_f16")
    return out


def attn_probs(q, k, heads, scale, out=None):
    """materialised maps [B*heads, N, L] fp16 for the generic controller path (out: where to write them)."""
    if _is32(q):
        return _attn_scores_f32(q, k, heads, scale, out=out)
    lib = load()
    B, N, C = q.shape
    L = k.shape[1]
    if out is None:
        probs = torch.empty(B * heads, N, L, dtype=torch.float16, device=q.device)
    else:
        probs = _dev16(out, "out")
        if tuple(probs.shape) != (B * heads, N, L) or not probs.is_contiguous():
            raise ValueError("attn_probs: out must be contiguous fp16 [B*heads, N, L]")
    p = IefAttnParams()
    _attn_common(p, "attn_probs", q, k, k, q, heads)
    p.scale = scale
    _check(lib.ief_attn_probs_f16(byref(p), probs.data_ptr(), _stream()), "ief_attn_probs_f16")
    return probs


def attn_apply(probs, v, heads, out=None):
    """out [B,N,h*d] = probs [B*heads,N,L] @ v [B,L,h*d]."""
    if _is32(probs):
        return _attn_apply_f32(probs, v, heads, None, out)
    lib = load()
    _dev16(probs, "probs")
    if not probs.is_contiguous():
        raise ValueError("attn_apply: probs must be contiguous")
    B = v.shape[0]
    N, L = probs.shape[1], probs.shape[2]
    if probs.shape[0] != B * heads or v.shape[1] != L:
        raise ValueError("attn_apply: shape mismatch")
    if out is None:
        out = torch.empty(B, N, v.shape[2], dtype=torch.float16, device=v.device)
    p = IefAttnParams()
    if _attn_common(p, "attn_apply", out, v, v, out, heads).N != N:
        raise ValueError("attn_apply: out must have the maps' rows")
    _check(lib.ief_attn_apply_f16(byref(p), probs.data_ptr(), _stream()), "ief_attn_apply_f16")
    return out


# ------------------------------------------------------------------------------- sampler
PROX_MODES = {"l0": 0, "l1": 1}      # the `mode` argument of ief_cfg_ddim_step_prox_f32
PROX_MAX_ROW = 65536                 # the longest row ief_prox_threshold_f32 selects over


def prox_threshold(eps_u, eps_c, rank, out=None):
    """proximal guidance's per-row threshold (`ief_prox_threshold_f32`): out[b] = the quantile of |eps_c[b] - eps_u[b]| over the
    elements of batch row b, t = v_(lo) + frac (v_(lo + 1) - v_(lo)) with exact order statistics.  eps_u, eps_c device fp32
    [B, ...] of one shape, 1 .. 65536 elements per row; rank device fp32 [2] = [lo, frac] (`control.ledits_rank` of the row
    length); out device fp32 [B]."""
    lib = load()
    _dev32(eps_u, "eps_u")
    _dev32(eps_c, "eps_c")
    if eps_u.dim() < 1 or eps_u.shape != eps_c.shape or eps_u.numel() == 0:
        raise ValueError(f"prox_threshold: eps_u and eps_c must be [B, ...] of one shape, got {tuple(eps_u.shape)} and "
                         f"{tuple(eps_c.shape)}")
    B, n = eps_u.shape[0], eps_u[0].numel()
    if not 1 <= n <= PROX_MAX_ROW:
        raise ValueError(f"prox_threshold: a row holds 1 .. {PROX_MAX_ROW} elements, got {n}")
    if _dev32(rank, "rank").numel() != 2:
        raise ValueError(f"prox_threshold: rank is [lo, frac], one pair for every row, got {tuple(rank.shape)}")
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=eps_u.device)
    if _dev32(out, "out").numel() != B:
        raise ValueError(f"prox_threshold: out must hold {B} elements")
    _check(lib.ief_prox_threshold_f32(eps_u.data_ptr(), eps_c.data_ptr(), rank.data_ptr(), out.data_ptr(), B, n, _stream()),
           "ief_prox_threshold_f32")
    return out


def cfg_ddim_step(eps_u, eps_c, x, coef, out=None, x0_out=None, rect=None, masked=None, prox=None):
    """x' from (eps_u, eps_c, x) with coef = device fp32 [a_from, a_to, guidance]; eps_u None => no CFG.
    prox = (thres, z0, mode, radius): the step under proximal guidance (`ief_cfg_ddim_step_prox_f32`) -- x [Bp, C, h, w], coef
    device fp32 [a_from, a_to, g, prox_on, eta], thres device fp32 [Bp] (`prox_threshold`), z0 device fp32 [C, h, w] the encoded
    source, mode "l0" / "l1", radius 0 .. 3 the dilation of the edit mask.  Row 0 is the plain step's bit for bit.
    rect = (traj, step): Direct Inversion in the same launch -- batch row 0 of x [Bp, ...] becomes x'[0] + (z - x'[0]) with
    z = traj[clamp(step[0], 0, S - 1)]; traj device fp32 [S, *x.shape[1:]], step device int32 [1] (read by the kernel).
    masked = (traj, step, mask): DiffEdit in the same launch -- x [Bp, C, h, w]; row b keeps x'[b] where mask[b] != 0 and takes
    z = traj[clamp(step[0], 0, rows - 1)] elsewhere (a select); mask device fp32 [Bp, h, w], traj device fp32 [rows, C, h, w]."""
    lib = load()
    _dev32(eps_c, "eps_c")
    _dev32(x, "x")
    _dev32(coef, "coef")
    if prox is not None:
        if rect is not None or masked is not None:
            raise ValueError("cfg_ddim_step: prox and rect / masked are different steps; choose one")
        thres, z0, mode, radius = prox
        if eps_u is None:
            raise ValueError("cfg_ddim_step: a proximal step thresholds eps_c - eps_u; it needs eps_u")
        _dev32(eps_u, "eps_u")
        _dev32(thres, "prox thresholds")
        _dev32(z0, "prox source latent")
        if x.dim() != 4 or eps_c.shape != x.shape or eps_u.shape != x.shape:
            raise ValueError(f"cfg_ddim_step: a proximal step takes eps_u, eps_c and x as [Bp, C, h, w] of one shape, got "
                             f"{tuple(eps_u.shape)}, {tuple(eps_c.shape)} and {tuple(x.shape)}")
        if coef.numel() != 5:
            raise ValueError(f"cfg_ddim_step: a proximal step's coef is [a_from, a_to, g, prox_on, eta], got {coef.numel()} elements")
        if thres.numel() != x.shape[0]:
            raise ValueError(f"cfg_ddim_step: {thres.numel()} thresholds for {x.shape[0]} batch rows")
        if tuple(z0.shape[-3:]) != tuple(x.shape[1:]) or z0.numel() != x[0].numel():
            raise ValueError(f"cfg_ddim_step: the source latent must be [{', '.join(map(str, x.shape[1:]))}], got {tuple(z0.shape)}")
        if mode not in PROX_MODES:
            raise ValueError(f"cfg_ddim_step: the proximal mode is one of {sorted(PROX_MODES)}, got {mode!r}")
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= 3:
            raise ValueError(f"cfg_ddim_step: the dilation radius is an integer in [0, 3], got {radius!r}")
        if x[0].numel() > PROX_MAX_ROW:
            raise ValueError(f"cfg_ddim_step: a proximal step serves rows of at most {PROX_MAX_ROW} elements, got {x[0].numel()}")
        if out is None:
            out = torch.empty_like(x)
        for t, name in ((out, "out"), (x0_out, "x0_out")):
            if t is not None and (_dev32(t, name).shape != x.shape):
                raise ValueError(f"cfg_ddim_step: {name} must have the shape of x")
        _check(lib.ief_cfg_ddim_step_prox_f32(eps_u.data_ptr(), eps_c.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out),
                                              coef.data_ptr(), thres.data_ptr(), z0.data_ptr(), x.numel(), x[0].numel(),
                                              x.shape[2], x.shape[3], PROX_MODES[mode], radius, _stream()),
               "ief_cfg_ddim_step_prox_f32")
        return out
    if masked is not None:
        if rect is not None:
            raise ValueError("cfg_ddim_step: rect and masked are two different steps; choose one")
        traj, step, mask = masked
        _dev32(traj, "masked trajectory")
        _dev32(mask, "mask")
        if eps_u is not None:
            _dev32(eps_u, "eps_u")
        if x.dim() != 4 or eps_c.shape != x.shape or (eps_u is not None and eps_u.shape != x.shape):
            raise ValueError(f"cfg_ddim_step: a masked step takes eps and x as [Bp, C, h, w] of one shape, got {tuple(eps_c.shape)} and "
                             f"{tuple(x.shape)}")
        if traj.dim() != 4 or traj.shape[0] < 1 or traj.shape[1:] != x.shape[1:]:
            raise ValueError(f"cfg_ddim_step: the trajectory must be [steps, {', '.join(map(str, x.shape[1:]))}] (x without its batch "
                             f"dimension), got {tuple(traj.shape)}")
        if tuple(mask.shape) != (x.shape[0], *x.shape[2:]):
            raise ValueError(f"cfg_ddim_step: the mask must be [{x.shape[0]}, {x.shape[2]}, {x.shape[3]}] (one per batch row), got "
                             f"{tuple(mask.shape)}")
        if _devi32(step, "masked step") is None or step.numel() != 1:
            raise TypeError("masked step: expected a device int32 tensor of one element")
        if out is None:
            out = torch.empty_like(x)
        for t, name in ((out, "out"), (x0_out, "x0_out")):
            if t is not None and (_dev32(t, name).shape != x.shape):
                raise ValueError(f"cfg_ddim_step: {name} must have the shape of x")
        _check(lib.ief_cfg_ddim_step_masked_f32(_ptr(eps_u), eps_c.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out),
                                                coef.data_ptr(), x.numel(), x[0].numel(), x.shape[2] * x.shape[3], traj.data_ptr(),
                                                traj.shape[0], step.data_ptr(), mask.data_ptr(), _stream()),
               "ief_cfg_ddim_step_masked_f32")
        return out
    if out is None:
        out = torch.empty_like(x)
    if rect is not None:
        traj, step = rect
        _dev32(traj, "rect trajectory")
        if x.dim() < 2 or traj.dim() != x.dim() or traj.shape[0] < 1 or traj.shape[1:] != x.shape[1:]:
            raise ValueError(f"cfg_ddim_step: the trajectory must be [steps, {', '.join(map(str, x.shape[1:]))}] (x without its batch "
                             f"dimension), got {tuple(traj.shape)}")
        if _devi32(step, "rect step") is None or step.numel() != 1:
            raise TypeError("rect step: expected a device int32 tensor of one element")
        _check(lib.ief_cfg_ddim_step_rect_f32(_ptr(eps_u), eps_c.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out),
                                              coef.data_ptr(), x.numel(), x[0].numel(), traj.data_ptr(), traj.shape[0],
                                              step.data_ptr(), _stream()), "ief_cfg_ddim_step_rect_f32")
        return out
    _check(lib.ief_cfg_ddim_step_f32(_ptr(eps_u), eps_c.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out),
                                     coef.data_ptr(), x.numel(), _stream()), "ief_cfg_ddim_step_f32")
    return out


def cfg_ddpm_step(eps_u, eps_c, x, coef, g_rows, noise, step, out=None, x0_out=None):
    """The eta = 1 step of an edit-friendly DDPM inversion edit (`ief_cfg_ddpm_step_f32`): for batch row b of x [Bp, ...]
        eps = eps_u[b] + g_rows[b] (eps_c[b] - eps_u[b]);  mu = sqrt(a_to) x0 + dir eps;  x'[b] = mu + sigma noise[clamp(step[0])]
    coef = device fp32 [a_from, a_to, sigma, dir]; g_rows device fp32 [Bp] (None only with eps_u None => eps = eps_c); noise device fp32
    [rows, *x.shape[1:]] -- every batch row reads the same row; step device int32 [1] (read by the kernel)."""
    lib = load()
    _dev32(eps_c, "eps_c")
    _dev32(x, "x")
    _dev32(coef, "coef")
    _dev32(noise, "noise maps")
    if eps_u is not None:
        _dev32(eps_u, "eps_u")
        _dev32(g_rows, "g_rows")
    if x.dim() < 2 or eps_c.shape != x.shape or (eps_u is not None and eps_u.shape != x.shape):
        raise ValueError(f"cfg_ddpm_step: eps and x must be [Bp, ...] of one shape, got {tuple(eps_c.shape)} and {tuple(x.shape)}")
    if coef.numel() != 4:
        raise ValueError(f"cfg_ddpm_step: coef is [a_from, a_to, sigma, dir], got {coef.numel()} elements")
    if eps_u is not None and g_rows.numel() != x.shape[0]:
        raise ValueError(f"cfg_ddpm_step: {g_rows.numel()} guidance scales for {x.shape[0]} batch rows")
    if noise.dim() != x.dim() or noise.shape[0] < 1 or noise.shape[1:] != x.shape[1:]:
        raise ValueError(f"cfg_ddpm_step: the noise maps must be [steps, {', '.join(map(str, x.shape[1:]))}] (x without its batch "
                         f"dimension), got {tuple(noise.shape)}")
    if _devi32(step, "step") is None or step.numel() != 1:
        raise TypeError("step: expected a device int32 tensor of one element")
    if out is None:
        out = torch.empty_like(x)
    for t, name in ((out, "out"), (x0_out, "x0_out")):
        if t is not None and (_dev32(t, name).shape != x.shape):
            raise ValueError(f"cfg_ddpm_step: {name} must have the shape of x")
    _check(lib.ief_cfg_ddpm_step_f32(_ptr(eps_u), eps_c.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out), coef.data_ptr(),
                                     _ptr(g_rows) if eps_u is not None else None, x.numel(), x[0].numel(), noise.data_ptr(),
                                     noise.shape[0], step.data_ptr(), _stream()), "ief_cfg_ddpm_step_f32")
    return out


def ddpm_noise_maps(eps_u, eps_c, x_t, x_prev, coef_rows, out=None):
    """The noise maps of R rows at R timesteps in one launch (`ief_ddpm_noise_maps_f32`): z[r] = (x_prev[r] - mu_r) / sigma_r with
    mu_r the mean of `cfg_ddpm_step` at (x_t[r], eps[r]); a row with sigma_r == 0 is zero.  All tensors device fp32 [R, ...];
    coef_rows device fp32 [R, 5] = [a_from, a_to, sigma, dir, guidance] per row; eps_u None => eps = eps_c."""
    lib = load()
    for t, name in ((eps_c, "eps_c"), (x_t, "x_t"), (x_prev, "x_prev"), (coef_rows, "coef_rows")) + (
            () if eps_u is None else ((eps_u, "eps_u"),)) + (() if out is None else ((out, "out"),)):
        _dev32(t, name)
    if x_t.dim() < 2 or any(t.shape != x_t.shape for t in (eps_c, x_prev) + (() if eps_u is None else (eps_u,)) +
                            (() if out is None else (out,))):
        raise ValueError(f"ddpm_noise_maps: eps, x_t, x_prev and out must be [R, ...] of one shape ({tuple(x_t.shape)})")
    if tuple(coef_rows.shape) != (x_t.shape[0], 5):
        raise ValueError(f"ddpm_noise_maps: coef_rows must be [{x_t.shape[0]}, 5] = [a_from, a_to, sigma, dir, guidance] per row, "
                         f"got {tuple(coef_rows.shape)}")
    if out is None:
        out = torch.empty_like(x_t)
    _check(lib.ief_ddpm_noise_maps_f32(_ptr(eps_u), eps_c.data_ptr(), x_t.data_ptr(), x_prev.data_ptr(), out.data_ptr(),
                                       coef_rows.data_ptr(), x_t.shape[0], x_t[0].numel(), _stream()), "ief_ddpm_noise_maps_f32")
    return out


def cfg_dpmpp_step(eps_u, eps_c, x, coef, g_rows, noise, step, x0_prev, out=None, x0_out=None):
    """`cfg_ddpm_step` at solver order 2 (`ief_cfg_dpmpp_step_f32`, second-order multistep SDE-DPM-Solver++):
        mu = sqrt(a_to) x0 + dir eps + c2 (x0 - x0_prev);  x'[b] = mu + sigma noise[clamp(step[0])];  x0_prev := x0
    coef = device fp32 [a_from, a_to, sigma, dir, c2] (`DDIMScheduler.dpmpp_coeffs`); x0_prev device fp32 of x's shape, updated in
    place -- with c2 == 0 it is not read into the result and the outputs are `cfg_ddpm_step`'s bit for bit.  Everything else as
    there."""
    lib = load()
    _dev32(eps_c, "eps_c")
    _dev32(x, "x")
    _dev32(coef, "coef")
    _dev32(noise, "noise maps")
    if eps_u is not None:
        _dev32(eps_u, "eps_u")
        _dev32(g_rows, "g_rows")
    if x.dim() < 2 or eps_c.shape != x.shape or (eps_u is not None and eps_u.shape != x.shape):
        raise ValueError(f"cfg_dpmpp_step: eps and x must be [Bp, ...] of one shape, got {tuple(eps_c.shape)} and {tuple(x.shape)}")
    if coef.numel() != 5:
        raise ValueError(f"cfg_dpmpp_step: coef is [a_from, a_to, sigma, dir, c2], got {coef.numel()} elements")
    if eps_u is not None and g_rows.numel() != x.shape[0]:
        raise ValueError(f"cfg_dpmpp_step: {g_rows.numel()} guidance scales for {x.shape[0]} batch rows")
    if noise.dim() != x.dim() or noise.shape[0] < 1 or noise.shape[1:] != x.shape[1:]:
        raise ValueError(f"cfg_dpmpp_step: the noise maps must be [steps, {', '.join(map(str, x.shape[1:]))}] (x without its batch "
                         f"dimension), got {tuple(noise.shape)}")
    if _devi32(step, "step") is None or step.numel() != 1:
        raise TypeError("step: expected a device int32 tensor of one element")
    if x0_prev is None or _dev32(x0_prev, "x0_prev").shape != x.shape:
        raise ValueError("cfg_dpmpp_step: x0_prev must have the shape of x")
    if out is None:
        out = torch.empty_like(x)
    for t, name in ((out, "out"), (x0_out, "x0_out")):
        if t is not None and (_dev32(t, name).shape != x.shape):
            raise ValueError(f"cfg_dpmpp_step: {name} must have the shape of x")
    _check(lib.ief_cfg_dpmpp_step_f32(_ptr(eps_u), eps_c.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out), x0_prev.data_ptr(),
                                      coef.data_ptr(), _ptr(g_rows) if eps_u is not None else None, x.numel(), x[0].numel(),
                                      noise.data_ptr(), noise.shape[0], step.data_ptr(), _stream()), "ief_cfg_dpmpp_step_f32")
    return out


def dpmpp_noise_maps(eps_u, eps_c, x_t, x_prev, coef_rows, x0_carry, out=None):
    """`ddpm_noise_maps` under the order-2 mean (`ief_dpmpp_noise_maps_f32`): the R rows are CONSECUTIVE timesteps of one image,
    z[r] = (x_prev[r] - mu_r) / sigma_r with mu_r = mu1_r + c2_r (x0_r - x0_{r-1}), x0_r the x0 prediction of row r's own eps.
    coef_rows device fp32 [R, 6] = [a_from, a_to, sigma, dir, guidance, c2] per row; x0_carry device fp32 of one row's shape: the
    x0 of the row before row 0 (not read into the result where c2_0 == 0), overwritten with row R - 1's -- so chunks launched in
    order give the bits of one launch."""
    lib = load()
    for t, name in ((eps_c, "eps_c"), (x_t, "x_t"), (x_prev, "x_prev"), (coef_rows, "coef_rows")) + (
            () if eps_u is None else ((eps_u, "eps_u"),)) + (() if out is None else ((out, "out"),)):
        _dev32(t, name)
    if x_t.dim() < 2 or any(t.shape != x_t.shape for t in (eps_c, x_prev) + (() if eps_u is None else (eps_u,)) +
                            (() if out is None else (out,))):
        raise ValueError(f"dpmpp_noise_maps: eps, x_t, x_prev and out must be [R, ...] of one shape ({tuple(x_t.shape)})")
    if tuple(coef_rows.shape) != (x_t.shape[0], 6):
        raise ValueError(f"dpmpp_noise_maps: coef_rows must be [{x_t.shape[0]}, 6] = [a_from, a_to, sigma, dir, guidance, c2] per "
                         f"row, got {tuple(coef_rows.shape)}")
    if x0_carry is None or _dev32(x0_carry, "x0_carry").shape != x_t.shape[1:]:
        raise ValueError(f"dpmpp_noise_maps: x0_carry must be one row [{', '.join(map(str, x_t.shape[1:]))}]")
    if out is None:
        out = torch.empty_like(x_t)
    _check(lib.ief_dpmpp_noise_maps_f32(_ptr(eps_u), eps_c.data_ptr(), x_t.data_ptr(), x_prev.data_ptr(), out.data_ptr(),
                                        coef_rows.data_ptr(), x0_carry.data_ptr(), x_t.shape[0], x_t[0].numel(), _stream()),
           "ief_dpmpp_noise_maps_f32")
    return out


def diffedit_map_accum(eps_a, eps_b, acc):
    """DiffEdit's difference map (`ief_diffedit_map_accum_f32`): acc[p] += sum_r sum_c |eps_a[r, c, p] - eps_b[r, c, p]| in row and
    channel order, every operation rounded in fp32 -- chunking the rows over launches does not change a bit.  eps_a, eps_b device
    fp32 [R, C, h, w]; acc device fp32 [h, w], updated in place (the caller zeroes it before the first chunk)."""
    lib = load()
    for t, name in ((eps_a, "eps_a"), (eps_b, "eps_b"), (acc, "acc")):
        _dev32(t, name)
    if eps_a.dim() != 4 or eps_a.shape[0] < 1 or eps_b.shape != eps_a.shape:
        raise ValueError(f"diffedit_map_accum: eps_a and eps_b must be [R, C, h, w] of one shape, got {tuple(eps_a.shape)} and "
                         f"{tuple(eps_b.shape)}")
    if tuple(acc.shape) != tuple(eps_a.shape[2:]):
        raise ValueError(f"diffedit_map_accum: acc must be [{eps_a.shape[2]}, {eps_a.shape[3]}], got {tuple(acc.shape)}")
    _check(lib.ief_diffedit_map_accum_f32(eps_a.data_ptr(), eps_b.data_ptr(), acc.data_ptr(), eps_a.shape[0], eps_a.shape[1],
                                          acc.numel(), _stream()), "ief_diffedit_map_accum_f32")
    return acc


def diffedit_mask(acc, count: int, ratio: float = 3.0, thres: float = 0.5, out=None):
    """DiffEdit's mask rule (`ief_diffedit_mask_f32`): d = acc / count, v = min(max(d, 0), ratio mean(d)) / (ratio mean(d)),
    out = 1.0 where v > thres else 0.0; a zero map gives a zero mask.  acc device fp32 [h, w]; out device fp32 of acc's shape."""
    lib = load()
    _dev32(acc, "acc")
    if acc.numel() < 1:
        raise ValueError("diffedit_mask: acc has no elements")
    if not isinstance(count, int) or isinstance(count, bool) or count < 1:
        raise ValueError(f"diffedit_mask: count must be a positive integer, got {count!r}")
    if out is None:
        out = torch.empty_like(acc)
    if _dev32(out, "out").shape != acc.shape or out.data_ptr() == acc.data_ptr():
        raise ValueError("diffedit_mask: out must have acc's shape and its own memory")
    _check(lib.ief_diffedit_mask_f32(acc.data_ptr(), out.data_ptr(), acc.numel(), count, float(ratio), float(thres), _stream()),
           "ief_diffedit_mask_f32")
    return out


def _ledits_rank(rank, E, who):
    if tuple(_dev32(rank, "rank").shape) != (E, 2):
        raise ValueError(f"{who}: rank must be [{E}, 2] = [lo, frac] per concept, got {tuple(rank.shape)}")
    return rank


def ledits_attn_mask(acc, taps, rank, out=None):
    """LEDITS++'s cross-attention mask M1 (`ief_ledits_attn_mask_f32`): per concept e the 16 x 16 mass acc[e] is smoothed with the
    nine `taps` (3 x 3, row-major tap order, reflect padding) and thresholded at its quantile,
        t = v_(lo) + frac (v_(lo + 1) - v_(lo));  out[e] = 1.0 where smoothed >= t else 0.0
    with exact order statistics.  acc device fp32 [E, 256] (or [E, 16, 16]), 1 <= E <= 8; taps device fp32 [9]; rank device fp32
    [E, 2] = [lo, frac] per concept (`ledits.rank_table`); out device fp32 of acc's shape, its own memory."""
    lib = load()
    _dev32(acc, "acc")
    _dev32(taps, "taps")
    if acc.dim() < 2 or acc[0].numel() != 256:
        raise ValueError(f"ledits_attn_mask: acc must be [E, 256], got {tuple(acc.shape)}")
    E = acc.shape[0]
    if taps.numel() != 9:
        raise ValueError(f"ledits_attn_mask: taps are the nine weights of a 3 x 3 filter, got {taps.numel()} elements")
    _ledits_rank(rank, E, "ledits_attn_mask")
    if out is None:
        out = torch.empty_like(acc)
    if _dev32(out, "out").shape != acc.shape or out.data_ptr() == acc.data_ptr():
        raise ValueError("ledits_attn_mask: out must have acc's shape and its own memory")
    _check(lib.ief_ledits_attn_mask_f32(acc.data_ptr(), taps.data_ptr(), rank.data_ptr(), out.data_ptr(), E, _stream()),
           "ief_ledits_attn_mask_f32")
    return out


def ledits_guidance_mask(eps, m1=None, rank=None, out=None, thres_out=None):
    """LEDITS++'s per-concept mask M (`ief_ledits_guidance_mask_f32`): for concept e and pixel p
        s[p] = sum_c |eps[1 + e, c, p] - eps[0, c, p]| m,  m = m1[e, cell(p)]  (1 without m1; cell = the 16 x 16 cell of p)
        t = the `rank[e]` quantile of s (exact order statistics);  out[e, p] = 1.0 where s[p] >= t and m != 0 else 0.0
    channels in order, every operation rounded in fp32.  rank None: no threshold, out is m1 spread to the pixels.  eps device fp32
    [1 + E, C, h, w], row 0 the unconditional estimate, h w <= 16384, C <= 16, 1 <= E <= 8 (h, w multiples of 16 with m1); m1 device
    fp32 [E, 256] of 0.0 / 1.0; rank device fp32 [E, 2]; out device fp32 [E, h, w]; thres_out device fp32 [E] receives t.
    Returns (out, thres_out); thres_out stays None (and unwritten) without rank."""
    lib = load()
    _dev32(eps, "eps")
    if eps.dim() != 4 or eps.shape[0] < 2:
        raise ValueError(f"ledits_guidance_mask: eps must be [1 + E, C, h, w] with E >= 1, got {tuple(eps.shape)}")
    E, C, H, W = eps.shape[0] - 1, eps.shape[1], eps.shape[2], eps.shape[3]
    if m1 is not None and (_dev32(m1, "m1").dim() < 2 or m1.shape[0] != E or m1[0].numel() != 256):
        raise ValueError(f"ledits_guidance_mask: m1 must be [{E}, 256], got {tuple(m1.shape)}")
    if rank is not None:
        _ledits_rank(rank, E, "ledits_guidance_mask")
        if thres_out is None:
            thres_out = torch.empty(E, dtype=torch.float32, device=eps.device)
        if _dev32(thres_out, "thres_out").numel() != E:
            raise ValueError(f"ledits_guidance_mask: thres_out must hold {E} elements")
    if out is None:
        out = torch.empty((E, H, W), dtype=torch.float32, device=eps.device)
    if tuple(_dev32(out, "out").shape) != (E, H, W):
        raise ValueError(f"ledits_guidance_mask: out must be [{E}, {H}, {W}], got {tuple(out.shape)}")
    _check(lib.ief_ledits_guidance_mask_f32(eps.data_ptr(), _ptr(m1), _ptr(rank), out.data_ptr(),
                                            _ptr(thres_out) if rank is not None else None, E, C, H, W, _stream()),
           "ief_ledits_guidance_mask_f32")
    return out, (thres_out if rank is not None else None)


def ledits_ddpm_step(eps, mask, scale, x, coef, noise, step, out=None, x0_out=None):
    """The step of a LEDITS++ edit on ONE latent (`ief_ledits_ddpm_step_f32`): with eps [1 + E, C, h, w], row 0 unconditional,
        eps' = eps[0] + sum_e scale[e] mask[e] (eps[1 + e] - eps[0]);  mu = sqrt(a_to) x0 + dir eps';  x' = mu + sigma noise[clamp(step[0])]
    the sum in concept order from 0, a concept with scale[e] == 0 skipped; the mean is `cfg_ddpm_step`'s (one device function), so E = 1
    without a mask IS that step.  mask device fp32 [E, h, w] or None (all ones); scale device fp32 [E] (sign and gate folded in);
    x device fp32 [1, C, h, w] or [C, h, w]; coef = device fp32 [a_from, a_to, sigma, dir]; noise device fp32 [rows, C, h, w]; step
    device int32 [1] (read by the kernel)."""
    lib = load()
    for t, name in ((eps, "eps"), (scale, "scale"), (x, "x"), (coef, "coef"), (noise, "noise maps")):
        _dev32(t, name)
    if eps.dim() != 4 or eps.shape[0] < 2:
        raise ValueError(f"ledits_ddpm_step: eps must be [1 + E, C, h, w] with E >= 1, got {tuple(eps.shape)}")
    E, hw = eps.shape[0] - 1, eps.shape[2] * eps.shape[3]
    if x.numel() != eps[0].numel() or tuple(x.shape[-3:]) != tuple(eps.shape[1:]):
        raise ValueError(f"ledits_ddpm_step: x is ONE latent [{', '.join(map(str, eps.shape[1:]))}], got {tuple(x.shape)}")
    if mask is not None and tuple(_dev32(mask, "mask").shape) != (E,) + tuple(eps.shape[2:]):
        raise ValueError(f"ledits_ddpm_step: mask must be [{E}, {eps.shape[2]}, {eps.shape[3]}], got {tuple(mask.shape)}")
    if scale.numel() != E:
        raise ValueError(f"ledits_ddpm_step: {scale.numel()} scales for {E} concepts")
    if coef.numel() != 4:
        raise ValueError(f"ledits_ddpm_step: coef is [a_from, a_to, sigma, dir], got {coef.numel()} elements")
    if noise.dim() != 4 or noise.shape[0] < 1 or noise.shape[1:] != eps.shape[1:]:
        raise ValueError(f"ledits_ddpm_step: the noise maps must be [steps, {', '.join(map(str, eps.shape[1:]))}], got "
                         f"{tuple(noise.shape)}")
    if _devi32(step, "step") is None or step.numel() != 1:
        raise TypeError("step: expected a device int32 tensor of one element")
    if out is None:
        out = torch.empty_like(x)
    for t, name in ((out, "out"), (x0_out, "x0_out")):
        if t is not None and (_dev32(t, name).shape != x.shape):
            raise ValueError(f"ledits_ddpm_step: {name} must have the shape of x")
    _check(lib.ief_ledits_ddpm_step_f32(eps.data_ptr(), _ptr(mask), scale.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out),
                                        coef.data_ptr(), x.numel(), hw, noise.data_ptr(), noise.shape[0], step.data_ptr(), E,
                                        _stream()), "ief_ledits_ddpm_step_f32")
    return out


def ledits_dpmpp_step(eps, mask, scale, x, coef, noise, step, x0_prev, out=None, x0_out=None):
    """`ledits_ddpm_step` at solver order 2 (`ief_ledits_dpmpp_step_f32`): the same masked multi-concept guidance, then the mean of
    `cfg_dpmpp_step` (one device function), mu = mu1 + c2 (x0 - x0_prev), x0_prev := x0.  coef = device fp32 [a_from, a_to, sigma,
    dir, c2]; x0_prev device fp32 of x's shape, updated in place; with c2 == 0 the outputs are `ledits_ddpm_step`'s bit for bit."""
    lib = load()
    for t, name in ((eps, "eps"), (scale, "scale"), (x, "x"), (coef, "coef"), (noise, "noise maps")):
        _dev32(t, name)
    if eps.dim() != 4 or eps.shape[0] < 2:
        raise ValueError(f"ledits_dpmpp_step: eps must be [1 + E, C, h, w] with E >= 1, got {tuple(eps.shape)}")
    E, hw = eps.shape[0] - 1, eps.shape[2] * eps.shape[3]
    if x.numel() != eps[0].numel() or tuple(x.shape[-3:]) != tuple(eps.shape[1:]):
        raise ValueError(f"ledits_dpmpp_step: x is ONE latent [{', '.join(map(str, eps.shape[1:]))}], got {tuple(x.shape)}")
    if mask is not None and tuple(_dev32(mask, "mask").shape) != (E,) + tuple(eps.shape[2:]):
        raise ValueError(f"ledits_dpmpp_step: mask must be [{E}, {eps.shape[2]}, {eps.shape[3]}], got {tuple(mask.shape)}")
    if scale.numel() != E:
        raise ValueError(f"ledits_dpmpp_step: {scale.numel()} scales for {E} concepts")
    if coef.numel() != 5:
        raise ValueError(f"ledits_dpmpp_step: coef is [a_from, a_to, sigma, dir, c2], got {coef.numel()} elements")
    if noise.dim() != 4 or noise.shape[0] < 1 or noise.shape[1:] != eps.shape[1:]:
        raise ValueError(f"ledits_dpmpp_step: the noise maps must be [steps, {', '.join(map(str, eps.shape[1:]))}], got "
                         f"{tuple(noise.shape)}")
    if _devi32(step, "step") is None or step.numel() != 1:
        raise TypeError("step: expected a device int32 tensor of one element")
    if x0_prev is None or _dev32(x0_prev, "x0_prev").numel() != x.numel():
        raise ValueError("ledits_dpmpp_step: x0_prev must hold one latent, as x")
    if out is None:
        out = torch.empty_like(x)
    for t, name in ((out, "out"), (x0_out, "x0_out")):
        if t is not None and (_dev32(t, name).shape != x.shape):
            raise ValueError(f"ledits_dpmpp_step: {name} must have the shape of x")
    _check(lib.ief_ledits_dpmpp_step_f32(eps.data_ptr(), _ptr(mask), scale.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(x0_out),
                                         x0_prev.data_ptr(), coef.data_ptr(), x.numel(), hw, noise.data_ptr(), noise.shape[0],
                                         step.data_ptr(), E, _stream()), "ief_ledits_dpmpp_step_f32")
    return out


def ddim_step(eps, x, a_from: float, a_to: float):
    """scheduler.step on device tensors: returns (x_prev, x0)."""
    coef = torch.tensor([a_from, a_to, 1.0], dtype=torch.float32, device=x.device)
    x0 = torch.empty_like(x, dtype=torch.float32)
    xf = x.float().contiguous()
    out = cfg_ddim_step(None, eps.float().contiguous(), xf, coef, x0_out=x0)
    return out, x0


def timestep_embedding(t, dim, dtype=torch.float16):
    lib = load()
    _dev32(t, "t")
    if dtype == torch.float32:
        out = torch.empty(t.shape[0], dim, dtype=torch.float32, device=t.device)
        _check(lib.ief_timestep_embedding_f32(t.data_ptr(), out.data_ptr(), t.shape[0], dim, _stream()),
               "ief_timestep_embedding_f32")
        return out
    out = torch.empty(t.shape[0], dim, dtype=torch.float16, device=t.device)
    _check(lib.ief_timestep_embedding_f16(t.data_ptr(), out.data_ptr(), t.shape[0], dim, _stream()),
           "ief_timestep_embedding_f16")
    return out


def silu(x):
    lib = load()
    if _is32(x):
        out = torch.empty_like(_act32(x, "x"))
        _check(lib.ief_silu_f32(x.contiguous().data_ptr(), out.data_ptr(), x.numel(), _stream()), "ief_silu_f32")
        return out
    _dev16(x, "x")
    out = torch.empty_like(x)
    _check(lib.ief_silu_f16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "ief_silu_f16")
    return out


def to_f16(x, out=None):
    lib = load()
    _dev32(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _check(lib.ief_cast_f32_to_f16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "ief_cast_f32_to_f16")
    return out


def to_f32(x, out=None):
    lib = load()
    _dev16(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _check(lib.ief_cast_f16_to_f32(x.contiguous().data_ptr(), out.data_ptr(), x.numel(), _stream()), "ief_cast_f16_to_f32")
    return out


def image_u8(x):
    """decoder output fp32 NCHW [B,C,H,W] in [-1, 1] -> uint8 NHWC [B,H,W,C] on the device:
    (x / 2 + 0.5).clamp(0, 1) * 255, truncated (`/root/reference/p2p/model/sd_utils.py:85-88`)"""
    lib = load()
    _dev32(x, "x")
    B, C, H, Wd = x.shape
    out = torch.empty(B, H, Wd, C, dtype=torch.uint8, device=x.device)
    _check(lib.ief_image_u8(x.data_ptr(), out.data_ptr(), B, C, H, Wd, _stream()), "ief_image_u8")
    return out


def select_step(table, out, step):
    """out[...] = table[clamp(step[0], 0, rows - 1), ...] inside the stream (graph-capturable); step: device int32 [1]."""
    lib = load()
    nbytes = out.numel() * out.element_size()
    if table[0].numel() * table.element_size() != nbytes or not table.is_contiguous() or not out.is_contiguous():
        raise ValueError("select_step: table[step] and out must have identical contiguous byte size")
    _check(lib.ief_select_step(table.data_ptr(), out.data_ptr(), _devi32(step, "step").data_ptr(), nbytes, table.shape[0],
                               _stream()), "ief_select_step")
    return out


def advance_step(step):
    lib = load()
    _check(lib.ief_advance_step(_devi32(step, "step").data_ptr(), _stream()), "ief_advance_step")


def cross_token_mass(q, k, heads, scale, rows, w, out):
    """out[r][n] = (1 / heads) sum_h sum_l w[r][l] softmax_l(scale q_h[rows[r]][n] . k_h[rows[r]][l]), r = 0, 1: the head-mean
    cross-attention map of two batch rows, summed over prompt tokens with multiplicities w, without the map (csrc/masa_auto.hip).
    q fp32 [B, N, heads*d], k fp32 [B, L, heads*d] (column slices are fine), w fp32 [2, L], out fp32 [2, N] (both contiguous);
    rows: two host ints.  d any multiple of 8, L <= 128."""
    lib = load()
    _act32(q, "q"), _act32(k, "k"), _dev32(w, "w"), _dev32(out, "out")
    B, N, C = q.shape
    L = k.shape[1]
    if q.dim() != 3 or k.dim() != 3 or k.shape[0] != B or k.shape[2] != C or C % heads:
        raise ValueError("cross_token_mass: q [B, N, heads*d] and k [B, L, heads*d]")
    r0, r1 = int(rows[0]), int(rows[1])
    if not (0 <= r0 < B and 0 <= r1 < B):
        raise ValueError(f"cross_token_mass: rows {tuple(rows)} outside the batch of {B}")
    if tuple(w.shape) != (2, L) or tuple(out.shape) != (2, N):
        raise ValueError(f"cross_token_mass: w must be [2, {L}] and out [2, {N}]")
    with _Timed("cross_token_mass_f32_kernel", 4.0 * heads * N * L * (C // heads), 4.0 * 2 * C * (N + L)):
        _check(lib.ief_cross_token_mass_f32(q.data_ptr(), k.data_ptr(), w.data_ptr(), out.data_ptr(), r0, r1, heads, N, L, C // heads,
                                            q.stride(1), k.stride(1), q.stride(0), k.stride(0), float(scale), _stream()),
               "ief_cross_token_mass_f32")
    return out


def masa_auto_classes(slots, c, thres, res, k_cls, q_cls, gate=None):
    """class bits of a res x res layer from the first c slots of `slots` (fp32 [K, 2, 256], what `cross_token_mass` wrote for the
    16 x 16 level): mean over the slots, per-row (v - min) / (max - min), nearest pixel, >= thres (device fp32 [1]); k_cls from row
    0 and q_cls from row 1, int32 [res*res / 32] holding one bit per token.  A row with max == min makes every token of both rows
    background.  gate (device int32 [1]): nothing is written while it holds 0."""
    lib = load()
    _dev32(slots, "slots"), _dev32(thres, "thres"), _devi32(k_cls, "k_cls"), _devi32(q_cls, "q_cls"), _devi32(gate, "gate")
    c, res = int(c), int(res)
    if slots.dim() != 3 or tuple(slots.shape[1:]) != (2, 256) or not 1 <= c <= slots.shape[0]:
        raise ValueError("masa_auto_classes: slots must be [K, 2, 256] with 1 <= c <= K")
    if (res * res) % 32 or k_cls.numel() != res * res // 32 or q_cls.numel() != res * res // 32:
        raise ValueError("masa_auto_classes: k_cls / q_cls hold res*res / 32 words each")
    _check(lib.ief_masa_auto_classes(slots.data_ptr(), c, thres.data_ptr(), res, k_cls.data_ptr(), q_cls.data_ptr(), _ptr(gate),
                                     _stream()), "ief_masa_auto_classes")


def cross_blend_mass(q, k, heads, scale, row0, w, acc):
    """acc[i][n] += (1 / heads) sum_h (sum_l v_i[l] softmax_l(scale q_h[row0+i][n] . k_h[row0+i][l]) + sum_l u_i[l] softmax_l(scale
    q_h[row0][n] . k_h[row0][l])): the head-mean EDITED cross-attention map of the prompt rows row0 .. row0 + Bp - 1, summed over
    the blend words, without the map (csrc/local_blend.hip).  q fp32 [B, N, heads*d], k fp32 [B, L, heads*d] (column slices are
    fine), w fp32 [Bp, 2, >= L] = (u_i, v_i) and acc fp32 [Bp, N] (both contiguous).  d any multiple of 8, L <= 128, Bp <= 8."""
    lib = load()
    _act32(q, "q"), _act32(k, "k"), _dev32(w, "w"), _dev32(acc, "acc")
    if q.dim() != 3 or k.dim() != 3 or k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2] or q.shape[2] % heads:
        raise ValueError("cross_blend_mass: q [B, N, heads*d] and k [B, L, heads*d]")
    B, N, C = q.shape
    L = k.shape[1]
    if w.dim() != 3 or w.shape[1] != 2 or w.shape[2] < L or acc.dim() != 2 or tuple(acc.shape) != (w.shape[0], N):
        raise ValueError(f"cross_blend_mass: w must be [Bp, 2, >= {L}] and acc [Bp, {N}]")
    Bp, row0 = w.shape[0], int(row0)
    if not (0 <= row0 and row0 + Bp <= B):
        raise ValueError(f"cross_blend_mass: rows {row0} .. {row0 + Bp - 1} outside the batch of {B}")
    with _Timed("cross_blend_mass_f32_kernel", 2.0 * (2 * Bp - 1) * heads * N * L * (C // heads), 4.0 * Bp * C * (N + L)):
        _check(lib.ief_cross_blend_mass_f32(q.data_ptr(), k.data_ptr(), w.data_ptr(), acc.data_ptr(), row0, Bp, heads, N, L, w.shape[2],
                                            C // heads, q.stride(1), k.stride(1), q.stride(0), k.stride(0), float(scale), _stream()),
               "ief_cross_blend_mass_f32")
    return acc


def local_blend(acc, thres, x):
    """LocalBlend's last lines on the device, in place on the latents x fp32 [Bp, C, H, W]: acc fp32 [Bp, 256] (what `cross_blend_mass`
    accumulated) -> 3 x 3 max pool, / image maximum, > thres (device fp32 [1]), mask_i |= mask_0, nearest pixel,
    x[i] = x[0] + m (x[i] - x[0]) for i >= 1.  H, W multiples of 16."""
    lib = load()
    _dev32(acc, "acc"), _dev32(thres, "thres"), _dev32(x, "x")
    if x.dim() != 4 or acc.dim() != 2 or tuple(acc.shape) != (x.shape[0], 256):
        raise ValueError("local_blend: x must be [Bp, C, H, W] and acc [Bp, 256]")
    Bp, C, H, W = x.shape
    _check(lib.ief_local_blend_f32(acc.data_ptr(), thres.data_ptr(), x.data_ptr(), Bp, C, H, W, _stream()), "ief_local_blend_f32")
    return x


def unpack_class_bits(words, n):
    """packed class words (int32, bit i of word w = token 32 w + i) -> bool [n] on the host"""
    w = words.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    return ((w[:, None] >> torch.arange(32)) & 1).flatten()[:n].bool()


def pack_class_bits(bits, device=None):
    """bool [n] (n a multiple of 32) -> packed int32 class words for `planes.attn_flash(q_cls= / k_cls=)`"""
    b = bits.detach().cpu().flatten().to(torch.int64)
    if b.numel() % 32:
        raise ValueError("pack_class_bits: the token count must be a multiple of 32")
    w = (b.reshape(-1, 32) << torch.arange(32)).sum(1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return w if device is None else w.to(device)


# ------------------------------------------------------------------------------- activation gradients (null-text inversion)
def map_loss_blocks(N, d):
    """loss partials per (batch, head) that `attn_map_loss_bwd` writes"""
    return load().ief_map_loss_blocks(int(N), int(d))


def attn_map_loss_bwd(q, k, ref, dq, heads, scale, gcoef, accumulate=True, loss=None, loss_coef=1.0):
    """Pix2Pix-zero map objective of one cross-attention module (include/ief_hip.h, IefMapLossParams): with
    P = softmax(scale q k^T) and e = P - ref,  dq (+)= gcoef * scale * (P * (e - sum_j e_j P_j)) k.
    q [B,N,h*d], k [B,L,h*d] (strided views ok), ref fp16 [B*heads,N,L];
    loss: optional fp32 [B*heads*map_loss_blocks(N, d)] partials of sum e^2 (each times loss_coef)."""
    lib = load()
    if _is32(q):
        return _attn_map_loss_bwd_f32(q, k, ref, dq, heads, scale, gcoef, accumulate, loss, loss_coef)
    _dev16(q, "q"), _dev16(k, "k"), _dev16(ref, "ref"), _dev16(dq, "dq")
    B, N, C = q.shape
    L = k.shape[1]
    d = C // heads
    if tuple(ref.shape) != (B * heads, N, L) or not ref.is_contiguous():
        raise ValueError("attn_map_loss_bwd: ref must be contiguous fp16 [B*heads, N, L]")
    if tuple(dq.shape) != (B, N, C) or k.shape[0] != B or k.shape[2] != C:
        raise ValueError("attn_map_loss_bwd: shape mismatch")
    for nm, t in (("q", q), ("k", k), ("dq", dq)):
        if t.stride(2) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
            raise ValueError(f"attn_map_loss_bwd: {nm} must be [B, rows, h*d] with batch stride rows * ld")
    p = IefMapLossParams()
    p.Q, p.K, p.ref, p.dQ = q.data_ptr(), k.data_ptr(), ref.data_ptr(), dq.data_ptr()
    p.B, p.heads, p.N, p.L, p.d = B, heads, N, L, d
    p.ldq, p.ldk, p.lddq = q.stride(1), k.stride(1), dq.stride(1)
    p.scale, p.gcoef, p.loss_coef, p.accumulate = scale, gcoef, loss_coef, 1 if accumulate else 0
    if loss is not None:
        if _dev32(loss, "loss").numel() < B * heads * lib.ief_map_loss_blocks(N, d):
            raise ValueError("attn_map_loss_bwd: loss needs B*heads*map_loss_blocks(N, d) floats")
        p.loss = loss.data_ptr()
    _check(lib.ief_attn_map_loss_bwd_f16(byref(p), _stream()), "ief_attn_map_loss_bwd_f16")
    return dq



# ------------------------------------------------------------------------------- attention gradients, fp32-storage modes
def _transpose_maps_f32(x):
    """[R, N, L] fp32 -> contiguous [R, L, N]"""
    lib = load()
    R, N, L = x.shape
    out = torch.empty(R, L, N, dtype=torch.float32, device=x.device)
    _check(lib.ief_transpose_batched_f32(_act32(x, "maps").data_ptr(), out.data_ptr(), R, N, L, _stream()), "ief_transpose_batched_f32")
    return out


def _attn_apply_t_f32(maps, x, heads, out=None):
    """out [B, L, heads*d] = maps[b, h]^T [L x N] @ x[b, h] [N x d] per (batch row, head) WITHOUT transposing the maps: the product
    is taken as (x^T maps)^T -- x^T [d x N] is the small A operand, the maps [N x L] are read in place as the [K][N] operand,
    and only the [d x L] result is transposed back (the explicit [R, N, L] -> [R, L, N] copy moved 2 x 537 MB per 64x64
    self-attention layer and gradient)"""
    lib = load()
    _act32(maps, "maps"), _act32(x, "x")
    B, N, Cx = x.shape
    d = Cx // heads
    L = maps.shape[2]
    if tuple(maps.shape) != (B * heads, N, L) or not maps.is_contiguous():
        raise ValueError("attn_apply_t: maps must be contiguous [B*heads, N, L]")
    xt = x.reshape(B, N, heads, d).permute(0, 2, 3, 1).contiguous()                    # [B, heads, d, N]
    tmp = torch.empty(B * heads, d, L, dtype=torch.float32, device=x.device)
    p = IefGemmF32Params()
    p.A, p.W, p.Out = xt.data_ptr(), maps.data_ptr(), tmp.data_ptr()
    p.M, p.N, p.K = d, L, N
    p.sAb, p.sAh, p.lda = heads * d * N, d * N, N
    p.sWb, p.sWh, p.ldw = heads * N * L, N * L, L
    p.sOb, p.sOh, p.ldo = heads * d * L, d * L, L
    p.batch, p.heads, p.out_scale, p.transb = B, heads, 1.0, 1
    kn = _set_x3(p, X3_SCALE_ACT, X3_SCALE_PROB)
    with _Timed(f"{kn}<apply^T {d}>", 2.0 * B * heads * N * L * d, 4.0 * B * heads * (N * d + L * d + N * L)):
        _check(lib.ief_gemm_f32(byref(p), _stream()), "ief_gemm_f32 (attention apply, transposed maps)")
    res = tmp.reshape(B, heads, d, L).permute(0, 3, 1, 2).reshape(B, L, heads * d)
    if out is None:
        return res.contiguous()
    out.copy_(res)
    return out


def _softmax_bwd_f32_(probs, dprobs, scale):
    """in place on dprobs: dS = scale * P o (dP - rowsum(dP o P))"""
    lib = load()
    L = probs.shape[-1]
    _check(lib.ief_softmax_bwd_rows_f32(probs.data_ptr(), dprobs.data_ptr(), probs.numel() // L, L, float(scale), _stream()),
           "ief_softmax_bwd_rows_f32")
    return dprobs


def _attn_bwd_x3(q, k, v, o, do, lse, heads, scale, dq, dk, dv, want_dq, want_dkv):
    lib = load()
    B, N, L, _, d = _attn_geometry_of(_act32, "attn_bwd", q, k, v, heads, do=do, o=o, lse=_shape(_dev32(lse, "lse")))
    p = IefAttnBwdF32Params()
    what = 0
    if want_dq:
        dq = _grad_like(q, dq, "dq", "attn_bwd")
        p.dQ, p.lddq = dq.data_ptr(), dq.stride(1)
        what |= 1
    if want_dkv:
        dk, dv = _grad_like(k, dk, "dk", "attn_bwd"), _grad_like(v, dv, "dv", "attn_bwd")
        p.dK, p.dV, p.lddk, p.lddv = dk.data_ptr(), dv.data_ptr(), dk.stride(1), dv.stride(1)
        what |= 2
    delta = torch.empty(B, heads, N, dtype=torch.float32, device=q.device)
    _check(lib.ief_attn_bwd_delta_f32in(o.data_ptr(), do.data_ptr(), delta.data_ptr(), B, heads, N, d, o.stride(1), do.stride(1),
                                        _stream()), "ief_attn_bwd_delta_f32in")
    p.Q, p.K, p.V, p.dO, p.lse, p.delta = q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr()
    p.B, p.heads, p.N, p.L, p.d = B, heads, N, L, d
    p.ldq, p.ldk, p.ldv, p.ldo = q.stride(1), k.stride(1), v.stride(1), do.stride(1)
    p.scale, p.ds_mul = scale, X3_SCALE_PROB
    fl = (6.0 if want_dq else 0.0) + (8.0 if want_dkv else 0.0)
    with _Timed(f"attn_bwd_x3_kernel<{d}>", fl * B * heads * N * L * d):
        _check(lib.ief_attn_bwd_x3(byref(p), what, _stream()), "ief_attn_bwd_x3")
    return dq, dk, dv


def _attn_bwd_f32(q, k, v, do, heads, scale, dq, dk, dv, want_dq, want_dkv, o=None, lse=None):
    """gradients of softmax(scale q k^T) v on MATERIALISED fp32 maps (`/root/reference/p2p/model/register.py:43-51` is the
    forward being differentiated): P recomputed, dP = dO V^T, dS, then dQ = dS K, dK = dS^T Q, dV = P^T dO -- every
    product an `ief_gemm_f32` launch in the model's contraction mode.  With the forward's `lse` (split-operand mode, head dims
    40 / 64, >= 128 keys: `x3_fused_bwd_ok`) the fused recomputing kernel runs instead and no map is written.  Where dK / dV are
    wanted of an attention with few keys (`cross_bwd_ok`: the 77-key cross-attention of the null-text pass, in both contraction
    modes) `cross_bwd` gives all three gradients in plain fp32, again without a map."""
    d, L = q.shape[2] // heads, k.shape[1]
    if lse is not None and o is not None and x3_fused_bwd_ok(d, L):
        return _attn_bwd_x3(q, k, v, o, do, lse, heads, scale, dq, dk, dv, want_dq, want_dkv)
    if want_dkv and cross_bwd_ok(d, L, q.dtype) and not x3_fused_bwd_ok(d, L):
        return cross_bwd(q, k, v, do, heads, scale, dq=dq, dk=dk, dv=dv, want_dq=want_dq)
    _attn_geometry_of(_act32, "attn_bwd", q, k, v, heads, do=do)
    probs = _attn_scores_f32(q, k, heads, scale)                          # [B*h, N, L]
    ds = _attn_scores_f32(do, v, heads, 1.0, softmax=False)               # dP = dO V^T
    _softmax_bwd_f32_(probs, ds, scale)
    if want_dq:
        dq = _attn_apply_f32(ds, k, heads, out=dq)                        # dQ = dS K   (out: the caller's column slice, if any)
    if want_dkv:
        if ds.shape[2] % 4 == 0 and ds.shape[1] % 4 == 0:      # 16-byte rows of the [K][N] operand: every self-attention level
            dk = _attn_apply_t_f32(ds, q, heads, out=dk)                                # dK = dS^T Q
            dv = _attn_apply_t_f32(probs, do, heads, out=dv)                            # dV = P^T dO
        else:                                                  # 77 keys: the maps are small, transpose them
            dk = _attn_apply_f32(_transpose_maps_f32(ds), q, heads, out=dk)
            dv = _attn_apply_f32(_transpose_maps_f32(probs), do, heads, out=dv)
    return dq, dk, dv


def map_loss_blocks_f32(rows):
    return load().ief_map_loss_rows_blocks(rows)


def _attn_map_loss_bwd_f32(q, k, ref, dq, heads, scale, gcoef, accumulate, loss, loss_coef):
    """fp32 form of `attn_map_loss_bwd` on materialised maps: e = P - ref, dP = gcoef e, dS = scale P o (dP - sum dP P),
    dq (+)= dS k; loss: fp32 [map_loss_blocks_f32(B*heads*N)] partials"""
    lib = load()
    B, N, C = q.shape
    L = k.shape[1]
    if tuple(_act32(ref, "ref").shape) != (B * heads, N, L) or not ref.is_contiguous():
        raise ValueError("attn_map_loss_bwd: ref must be contiguous fp32 [B*heads, N, L]")
    probs = _attn_scores_f32(q, k, heads, scale)
    dp = torch.empty_like(probs)
    rows = B * heads * N
    if loss is not None and _dev32(loss, "loss").numel() < lib.ief_map_loss_rows_blocks(rows):
        raise ValueError("attn_map_loss_bwd: loss needs map_loss_blocks_f32(B*heads*N) floats")
    _check(lib.ief_map_loss_rows_f32(probs.data_ptr(), ref.data_ptr(), dp.data_ptr(), _ptr(loss), rows, L, float(gcoef),
                                     float(loss_coef), _stream()), "ief_map_loss_rows_f32")
    _softmax_bwd_f32_(probs, dp, scale)
    g = _attn_apply_f32(dp, k, heads)
    if accumulate:
        add(dq, g, out=dq)
    else:
        dq.copy_(g)
    return dq


def cross_map_grad_blocks(N, d):
    """loss partials per (batch, head) that `cross_map_grad` writes"""
    return load().ief_cross_map_grad_blocks(int(N), int(d))


def cross_map_grad(q, k, v, do, ref, heads, scale, gcoef, dq=None, loss=None, loss_coef=1.0):
    """Pix2Pix-zero guidance of one cross-attention module on the fp32-storage reverse pass, ONE launch (include/ief_hip.h,
    ief_attn_cross_map_grad_f32): with P = softmax(scale q k^T), dP = do v^T + gcoef (P - ref) and dS = P o (dP - rowsum(dP o P)),
    dq = scale dS k -- the gradient of the attention layer's value path and of the map objective together; dq is OVERWRITTEN.
    q / do [B,N,h*d], k / v [B,L,h*d] (strided views ok), ref fp32 [B*heads,N,L] contiguous; dq: None (allocated) or a view of
    q's shape; loss: optional fp32 [B*heads*cross_map_grad_blocks(N, d)] partials of sum (P - ref)^2, each times loss_coef."""
    lib = load()
    B, N, L, C, d = _attn_geometry_of(_act32, "cross_map_grad", q, k, v, heads, do=do)
    if tuple(_act32(ref, "ref").shape) != (B * heads, N, L) or not ref.is_contiguous():
        raise ValueError("cross_map_grad: ref must be contiguous fp32 [B*heads, N, L]")
    dq = _grad_like(q, dq, "dq", "cross_map_grad")
    if loss is not None and _dev32(loss, "loss").numel() < B * heads * lib.ief_cross_map_grad_blocks(N, d):
        raise ValueError("cross_map_grad: loss needs B*heads*cross_map_grad_blocks(N, d) floats")
    with _Timed(f"cross_map_grad_f32_kernel<{d}>", 6.0 * B * heads * N * L * d,
                4.0 * (3.0 * B * N * C + 2.0 * B * L * C + B * heads * N * L)):
        _check(lib.ief_attn_cross_map_grad_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr(), ref.data_ptr(), dq.data_ptr(),
                                               _ptr(loss), B, heads, N, L, d, q.stride(1), k.stride(1), v.stride(1), do.stride(1),
                                               dq.stride(1), float(scale), float(gcoef), float(loss_coef), _stream()),
               "ief_attn_cross_map_grad_f32")
    return dq


def cross_bwd_blocks(N, d):
    """dK / dV partials per (batch, head) that `cross_bwd`'s main kernel leaves for its reducer"""
    return load().ief_cross_bwd_blocks(int(N), int(d))


def cross_bwd(q, k, v, do, heads, scale, dq=None, dk=None, dv=None, want_dq=True):
    """The complete backward of out = softmax(scale q k^T) v for a short-key (cross-) attention on the fp32-storage reverse pass, no
    map in HBM (include/ief_hip.h, ief_attn_cross_bwd_f32): main kernel + reducer, fixed summation order, results OVERWRITTEN.
    q / do [B,N,h*d], k / v [B,L,h*d] (strided views ok); dq / dk / dv: None (allocated) or views of their operands' shapes, e.g.
    column slices of wider buffers; want_dq=False: dq is neither computed nor touched.  -> (dq or None, dk, dv)"""
    lib = load()
    B, N, L, C, d = _attn_geometry_of(_act32, "cross_bwd", q, k, v, heads, do=do)
    dq = _grad_like(q, dq, "dq", "cross_bwd") if want_dq else None
    dk, dv = _grad_like(k, dk, "dk", "cross_bwd"), _grad_like(v, dv, "dv", "cross_bwd")
    # the caller's scratch, as `delta` of ief_attn_bwd_x3: the caching allocator serves it under graph capture too
    scratch = torch.empty(max(1, lib.ief_cross_bwd_scratch_floats(B, heads, N, L, d)), dtype=torch.float32, device=q.device)
    with _Timed(f"cross_bwd_f32_kernel<{d}>", (10.0 if want_dq else 8.0) * B * heads * N * L * d,
                4.0 * ((3.0 if want_dq else 2.0) * B * N * C + 4.0 * B * L * C)):
        _check(lib.ief_attn_cross_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr(), _ptr(dq), dk.data_ptr(),
                                          dv.data_ptr(), scratch.data_ptr(), B, heads, N, L, d, q.stride(1), k.stride(1), v.stride(1),
                                          do.stride(1), dq.stride(1) if want_dq else 0, dk.stride(1), dv.stride(1), float(scale),
                                          _stream()), "ief_attn_cross_bwd_f32")
    return dq, dk, dv


def axpy(y, x, a):
    """y += a * x (fp32, in place)"""
    lib = load()
    _dev32(y, "y"), _dev32(x, "x")
    if y.shape != x.shape or not y.is_contiguous() or not x.is_contiguous():
        raise ValueError("axpy: operands must be contiguous and of equal shape")
    _check(lib.ief_axpy_f32(y.data_ptr(), x.data_ptr(), float(a), y.numel(), _stream()), "ief_axpy_f32")
    return y


def attn_bwd(q, k, v, o, do, lse, heads, scale, dq=None, dk=None, dv=None, ds_mul=None, want_dq=True, want_dkv=True):
    """Gradients of out = softmax(q k^T scale) v w.r.t. q, k, v given dO (`do`), the forward output `o` and its `lse`.
    q/do/o [B,N,h*d], k/v [B,L,h*d] (strided views ok); dq/dk/dv may be column slices of larger buffers."""
    lib = load()
    if _is32(q):
        return _attn_bwd_f32(q, k, v, do, heads, scale, dq, dk, dv, want_dq, want_dkv, o=o, lse=lse)
    p = IefAttnBwdParams()
    B, N, L, _, d = _attn_common(p, "attn_bwd", q, k, v, None, heads, do=do, o=o, lse=_shape(_dev32(lse, "lse")))
    delta = torch.empty(B, heads, N, dtype=torch.float32, device=q.device)
    _check(lib.ief_attn_bwd_delta_f32(o.data_ptr(), do.data_ptr(), delta.data_ptr(), B, heads, N, d, o.stride(1),
                                      do.stride(1), _stream()), "ief_attn_bwd_delta_f32")
    p.dO, p.ldo, p.lse, p.delta = do.data_ptr(), do.stride(1), lse.data_ptr(), delta.data_ptr()
    p.scale = scale
    p.ds_mul = float(ds_mul) if ds_mul is not None else float(min(L, 1024))
    what = 0
    if want_dq:
        dq = _grad_like(q, dq, "dq", "attn_bwd")
        p.dQ, p.lddq = dq.data_ptr(), dq.stride(1)
        what |= 1
    if want_dkv:
        dk, dv = _grad_like(k, dk, "dk", "attn_bwd"), _grad_like(v, dv, "dv", "attn_bwd")
        p.dK, p.dV, p.lddk, p.lddv = dk.data_ptr(), dv.data_ptr(), dk.stride(1), dv.stride(1)
        what |= 2
        # few keys (cross-attention) => few workgroups: cut the query range so ~256 of them run
        blocks, tiles = ((L + 127) // 128) * heads * B, (N + 63) // 64
        if blocks < 128 and tiles >= 4:
            p.kv_splits = max(1, min(tiles // 2, 256 // blocks))
            if p.kv_splits > 1:
                ws = torch.empty(2 * p.kv_splits * B * L * heads * d, dtype=torch.float32, device=q.device)
                p.ws = ws.data_ptr()
    fl = (6.0 if want_dq else 0.0) + (8.0 if want_dkv else 0.0)
    with _Timed(f"attn_bwd_kernel<{d}>", fl * B * heads * N * L * d):
        _check(lib.ief_attn_bwd_f16(byref(p), what, _stream()), "ief_attn_bwd_f16")
    return dq, dk, dv


def groupnorm_bwd(x, dy, gamma, beta, groups, eps, silu=False, x2=None, add=None, stats=None):
    """dx (and dx2 for a channel-concat input) of groupnorm(x | x2) [+ SiLU]; `add` is summed into the result.
    stats: (mean, rstd) [B, groups, 2] from `groupnorm(..., return_stats=True)` — enables the split two-launch path."""
    lib = load()
    if _is32(x):
        _act32(x, "x"), _act32(dy, "dy")
        B, C1 = x.shape[0], x.shape[-1]
        C2 = 0 if x2 is None else _act32(x2, "x2").shape[-1]
        HW = x.numel() // (B * C1)
        if not x.is_contiguous() or not dy.is_contiguous() or dy.numel() != B * HW * (C1 + C2) or (
                x2 is not None and (not x2.is_contiguous() or x2.numel() != B * HW * C2)) or (
                add is not None and (not _act32(add, "add").is_contiguous() or add.numel() != dy.numel())):
            raise ValueError("groupnorm_bwd: x / x2 / dy / add must be contiguous, dy and add [B, HW, C1+C2]")
        dx = torch.empty_like(x)
        dx2 = torch.empty_like(x2) if x2 is not None else None
        al16 = all(t is None or t.data_ptr() % 16 == 0 for t in (x, x2, dy, add, gamma, beta))
        if GN3_F32 and al16 and C1 % 4 == 0 and C2 % 4 == 0 and (C1 + C2) // groups <= 256:
            nws = lib.ief_groupnorm_bwd_f32_ws_floats(B, HW, C1 + C2)
            ws = torch.empty(nws, dtype=torch.float32, device=x.device)
            with _Timed("gn3_bwd_f32 (5 launches)", 0.0):
                _check(lib.ief_groupnorm_bwd_f32_ws(x.data_ptr(), _ptr(x2), C1, C2, dy.data_ptr(), _ptr(add), dx.data_ptr(), _ptr(dx2),
                                                    _dev32(gamma, "gamma").data_ptr(), _dev32(beta, "beta").data_ptr(), B, HW, groups,
                                                    eps, 1 if silu else 0, ws.data_ptr(), nws, _stream()), "ief_groupnorm_bwd_f32_ws")
            return (dx, dx2) if x2 is not None else dx
        with _Timed("gn_bwd_f32_kernel", 0.0):
            _check(lib.ief_groupnorm_bwd_f32(x.data_ptr(), _ptr(x2), C1, C2, dy.data_ptr(), _ptr(add), dx.data_ptr(), _ptr(dx2),
                                             _dev32(gamma, "gamma").data_ptr(), _dev32(beta, "beta").data_ptr(), B, HW, groups,
                                             eps, 1 if silu else 0, _stream()), "ief_groupnorm_bwd_f32")
        return (dx, dx2) if x2 is not None else dx
    _dev16(x, "x"), _dev16(dy, "dy")
    B, C1 = x.shape[0], x.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    HW = x.numel() // (B * C1)
    if not x.is_contiguous() or not dy.is_contiguous() or dy.numel() != B * HW * (C1 + C2):
        raise ValueError("groupnorm_bwd: x / dy must be contiguous, dy [B, HW, C1+C2]")
    if x2 is not None and (not _dev16(x2, "x2").is_contiguous() or x2.numel() != B * HW * C2):
        raise ValueError("groupnorm_bwd: x2 shape")
    if add is not None and (not _dev16(add, "add").is_contiguous() or add.numel() != dy.numel()):
        raise ValueError("groupnorm_bwd: add must match dy")
    dx = torch.empty_like(x)
    dx2 = torch.empty_like(x2) if x2 is not None else None
    partial = None
    if stats is not None:
        if tuple(_dev32(stats, "stats").shape) != (B, groups, 2):
            raise ValueError("groupnorm_bwd: stats must be fp32 [B, groups, 2]")
        partial = torch.empty(B * lib.ief_gn_splits(HW) * groups * 2, dtype=torch.float32, device=x.device)
    with _Timed("groupnorm_bwd", 0.0):
        _check(lib.ief_groupnorm_bwd_f16(x.data_ptr(), _ptr(x2), C1, C2, dy.data_ptr(), _ptr(add), dx.data_ptr(), _ptr(dx2),
                                         _dev32(gamma, "gamma").data_ptr(), _dev32(beta, "beta").data_ptr(), _ptr(stats),
                                         _ptr(partial), B, HW, groups, eps, 1 if silu else 0, _stream()),
               "ief_groupnorm_bwd_f16")
    return (dx, dx2) if x2 is not None else dx


def layernorm_bwd(x, dy, gamma, eps=1e-5, add=None):
    lib = load()
    if _is32(x):
        _act32(x, "x"), _act32(dy, "dy")
        if not x.is_contiguous() or not dy.is_contiguous() or dy.shape != x.shape or (
                add is not None and (not _act32(add, "add").is_contiguous() or add.shape != x.shape)):
            raise ValueError("layernorm_bwd: x / dy / add must be contiguous and of equal shape")
        C = x.shape[-1]
        dx = torch.empty_like(x)
        _check(lib.ief_layernorm_bwd_f32(x.data_ptr(), dy.data_ptr(), _ptr(add), dx.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                         x.numel() // C, C, eps, _stream()), "ief_layernorm_bwd_f32")
        return dx
    _dev16(x, "x"), _dev16(dy, "dy")
    if not x.is_contiguous() or not dy.is_contiguous() or dy.shape != x.shape:
        raise ValueError("layernorm_bwd: x / dy must be contiguous and of equal shape")
    if add is not None and (not _dev16(add, "add").is_contiguous() or add.shape != x.shape):
        raise ValueError("layernorm_bwd: add must match x")
    C = x.shape[-1]
    dx = torch.empty_like(x)
    _check(lib.ief_layernorm_bwd_f16(x.data_ptr(), dy.data_ptr(), _ptr(add), dx.data_ptr(), _dev32(gamma, "gamma").data_ptr(),
                                     x.numel() // C, C, eps, _stream()), "ief_layernorm_bwd_f16")
    return dx


def geglu_il(pre, out=None):
    """pre [..., 2*Ch] in the interleaved FF1 layout -> hidden * gelu(gate) [..., Ch]"""
    lib = load()
    if _is32(pre):
        if not _act32(pre, "pre").is_contiguous():
            raise ValueError("geglu_il: pre must be contiguous")
        Ch = pre.shape[-1] // 2
        if out is None:
            out = torch.empty(*pre.shape[:-1], Ch, dtype=torch.float32, device=pre.device)
        _check(lib.ief_geglu_il_f32(pre.data_ptr(), out.data_ptr(), pre.numel() // (2 * Ch), Ch, _stream()), "ief_geglu_il_f32")
        return out
    _dev16(pre, "pre")
    if not pre.is_contiguous():
        raise ValueError("geglu_il: pre must be contiguous")
    Ch = pre.shape[-1] // 2
    out = torch.empty(*pre.shape[:-1], Ch, dtype=torch.float16, device=pre.device)
    _check(lib.ief_geglu_il_f16(pre.data_ptr(), out.data_ptr(), pre.numel() // (2 * Ch), Ch, _stream()), "ief_geglu_il_f16")
    return out


def geglu_il_bwd(pre, dy):
    lib = load()
    if _is32(pre):
        _act32(pre, "pre"), _act32(dy, "dy")
        Ch = pre.shape[-1] // 2
        if not pre.is_contiguous() or not dy.is_contiguous() or dy.shape[-1] != Ch or dy.numel() * 2 != pre.numel():
            raise ValueError("geglu_il_bwd: pre [..., 2*Ch], dy [..., Ch], both contiguous")
        dpre = torch.empty_like(pre)
        _check(lib.ief_geglu_il_bwd_f32(pre.data_ptr(), dy.data_ptr(), dpre.data_ptr(), pre.numel() // (2 * Ch), Ch, _stream()),
               "ief_geglu_il_bwd_f32")
        return dpre
    _dev16(pre, "pre"), _dev16(dy, "dy")
    Ch = pre.shape[-1] // 2
    if not pre.is_contiguous() or not dy.is_contiguous() or dy.shape[-1] != Ch or dy.numel() * 2 != pre.numel():
        raise ValueError("geglu_il_bwd: pre [..., 2*Ch], dy [..., Ch], both contiguous")
    dpre = torch.empty_like(pre)
    _check(lib.ief_geglu_il_bwd_f16(pre.data_ptr(), dy.data_ptr(), dpre.data_ptr(), pre.numel() // (2 * Ch), Ch, _stream()),
           "ief_geglu_il_bwd_f16")
    return dpre


def zero_insert2x(x):
    """[B,H,W,C] -> [B,2H,2W,C] with x at the even positions, zeros elsewhere (stride-2 conv data gradient)"""
    lib = load()
    if _is32(x):
        if _act32(x, "x").dim() != 4 or not x.is_contiguous():
            raise ValueError("zero_insert2x: contiguous NHWC expected")
        B, H, W, C = x.shape
        out = torch.empty(B, 2 * H, 2 * W, C, dtype=torch.float32, device=x.device)
        _check(lib.ief_zero_insert2x_f32(x.data_ptr(), out.data_ptr(), B, H, W, C, _stream()), "ief_zero_insert2x_f32")
        return out
    _dev16(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("zero_insert2x: contiguous NHWC expected")
    B, H, W, C = x.shape
    out = torch.empty(B, 2 * H, 2 * W, C, dtype=torch.float16, device=x.device)
    _check(lib.ief_zero_insert2x_f16(x.data_ptr(), out.data_ptr(), B, H, W, C, _stream()), "ief_zero_insert2x_f16")
    return out


def pool2x2_sum(x):
    """[B,2H,2W,C] -> [B,H,W,C] summing each 2x2 block (nearest-2x upsample backward)"""
    lib = load()
    if _is32(x):
        if _act32(x, "x").dim() != 4 or not x.is_contiguous() or (x.shape[1] & 1) or (x.shape[2] & 1):
            raise ValueError("pool2x2_sum: contiguous NHWC with even H, W expected")
        B, H2, W2, C = x.shape
        out = torch.empty(B, H2 // 2, W2 // 2, C, dtype=torch.float32, device=x.device)
        _check(lib.ief_pool2x2_sum_f32(x.data_ptr(), out.data_ptr(), B, H2 // 2, W2 // 2, C, _stream()), "ief_pool2x2_sum_f32")
        return out
    _dev16(x, "x")
    if x.dim() != 4 or not x.is_contiguous() or (x.shape[1] & 1) or (x.shape[2] & 1):
        raise ValueError("pool2x2_sum: contiguous NHWC with even H, W expected")
    B, H2, W2, C = x.shape
    out = torch.empty(B, H2 // 2, W2 // 2, C, dtype=torch.float16, device=x.device)
    _check(lib.ief_pool2x2_sum_f16(x.data_ptr(), out.data_ptr(), B, H2 // 2, W2 // 2, C, _stream()), "ief_pool2x2_sum_f16")
    return out


def conv_out_bwd(d_eps, w):
    """d_eps fp32 NCHW [B,Cout,H,W], w fp16 [Cout,3,3,C] (conv_out's own weight) -> fp16 NHWC [B,H,W,C]"""
    lib = load()
    if _is32(w):
        _dev32(d_eps, "d_eps")
        B, Cout, H, W = d_eps.shape
        C = w.shape[-1]
        if tuple(_act32(w, "w").shape) != (Cout, 3, 3, C) or not w.is_contiguous():
            raise ValueError("conv_out_bwd: weight must be contiguous [Cout, 3, 3, C]")
        out = torch.empty(B, H, W, C, dtype=torch.float32, device=w.device)
        _check(lib.ief_conv_out_bwd_f32w(d_eps.data_ptr(), w.data_ptr(), out.data_ptr(), B, C, H, W, Cout, _stream()),
               "ief_conv_out_bwd_f32w")
        return out
    _dev32(d_eps, "d_eps"), _dev16(w, "w")
    B, Cout, H, W = d_eps.shape
    C = w.shape[-1]
    if tuple(w.shape) != (Cout, 3, 3, C) or not w.is_contiguous():
        raise ValueError("conv_out_bwd: weight must be contiguous [Cout, 3, 3, C]")
    out = torch.empty(B, H, W, C, dtype=torch.float16, device=w.device)
    _check(lib.ief_conv_out_bwd_f32(d_eps.data_ptr(), w.data_ptr(), out.data_ptr(), B, C, H, W, Cout, _stream()),
           "ief_conv_out_bwd_f32")
    return out


def nti_loss_grad(eps_u, eps_c, x, target, coef, d_eps, stats, grad_scale=1.0):
    """NTI objective + normalised gradient w.r.t. eps_u (see include/ief_hip.h); stats fp32 [2] <- (loss, factor)."""
    lib = load()
    for t, nm in ((eps_u, "eps_u"), (eps_c, "eps_c"), (x, "x"), (target, "target"), (coef, "coef"), (d_eps, "d_eps"),
                  (stats, "stats")):
        _dev32(t, nm)
    n = eps_u.numel()
    if any(t.numel() != n for t in (eps_c, x, target, d_eps)) or coef.numel() < 3 or stats.numel() < 2:
        raise ValueError("nti_loss_grad: shape mismatch")
    _check(lib.ief_nti_loss_grad_f32(eps_u.data_ptr(), eps_c.data_ptr(), x.data_ptr(), target.data_ptr(), coef.data_ptr(),
                                     d_eps.data_ptr(), stats.data_ptr(), n, grad_scale, _stream()), "ief_nti_loss_grad_f32")


def nti_adam(param, m, v, grad16, stats, hyper, step, param16):
    """One torch.optim.Adam step on fp32 `param` with g = grad16 * stats[1]; hyper fp32 {lr, beta1, beta2, eps}."""
    lib = load()
    for t, nm in ((param, "param"), (m, "m"), (v, "v"), (stats, "stats"), (hyper, "hyper")):
        _dev32(t, nm)
    if _is32(grad16):       # fp32-storage modes: the context IS the fp32 parameter (param16 unused)
        if grad16.numel() != param.numel() or not _act32(grad16, "grad").is_contiguous():
            raise ValueError("nti_adam: gradient shape mismatch")
        _check(lib.ief_nti_adam_f32g(param.data_ptr(), m.data_ptr(), v.data_ptr(), grad16.data_ptr(), stats.data_ptr(),
                                     hyper.data_ptr(), _devi32(step, "step").data_ptr(), param.numel(), _stream()),
               "ief_nti_adam_f32g")
        return
    _dev16(grad16, "grad16"), _dev16(param16, "param16")
    _devi32(step, "step")
    n = param.numel()
    if any(t.numel() != n for t in (m, v, grad16, param16)) or not grad16.is_contiguous() or not param16.is_contiguous():
        raise ValueError("nti_adam: shape mismatch")
    _check(lib.ief_nti_adam_f32(param.data_ptr(), m.data_ptr(), v.data_ptr(), grad16.data_ptr(), stats.data_ptr(),
                                hyper.data_ptr(), step.data_ptr(), param16.data_ptr(), n, _stream()), "ief_nti_adam_f32")


def nti_loss_grad_batched(eps_u, eps_c, x, target, coef, d_eps, stats, grad_scale=1.0):
    """`nti_loss_grad` for K images [K, ...] at one timestep (one `coef`): stats fp32 [K, 2] <- (loss, factor) per image;
    image k's d_eps and stats are bit-identical to `nti_loss_grad` on its slice."""
    lib = load()
    for t, nm in ((eps_u, "eps_u"), (eps_c, "eps_c"), (x, "x"), (target, "target"), (coef, "coef"), (d_eps, "d_eps"),
                  (stats, "stats")):
        _dev32(t, nm)
    K = eps_u.shape[0] if eps_u.dim() >= 2 else 0
    total = eps_u.numel()
    if K < 1 or any(t.numel() != total for t in (eps_c, x, target, d_eps)) or coef.numel() < 3 or tuple(stats.shape) != (K, 2):
        raise ValueError("nti_loss_grad_batched: operands must be [K, ...] of one shape, coef [>= 3], stats [K, 2]")
    _check(lib.ief_nti_loss_grad_batched_f32(eps_u.data_ptr(), eps_c.data_ptr(), x.data_ptr(), target.data_ptr(),
                                             coef.data_ptr(), d_eps.data_ptr(), stats.data_ptr(), total // K, K, grad_scale,
                                             _stream()), "ief_nti_loss_grad_batched_f32")


def nti_adam_batched(param, m, v, grad, stats, active, hyper, step, param16):
    """`nti_adam` for K parameters [K, ...] with one Adam state each, shared `hyper` and `step` (advanced once): image k
    takes g = grad[k] * stats[k, 1]; active int32 [K], an image with active[k] == 0 is left unwritten.  fp16 `grad` writes
    the fp16 copy `param16` too; an fp32 `grad` (fp32-storage modes) does not look at it."""
    lib = load()
    for t, nm in ((param, "param"), (m, "m"), (v, "v"), (stats, "stats"), (hyper, "hyper")):
        _dev32(t, nm)
    _devi32(step, "step"), _devi32(active, "active")
    K = param.shape[0] if param.dim() >= 2 else 0
    total = param.numel()
    if step is None or active is None:
        raise TypeError("nti_adam_batched: step and active are required")
    if K < 1 or any(t.numel() != total for t in (m, v, grad)) or tuple(stats.shape) != (K, 2) or active.numel() != K \
            or hyper.numel() < 4 or not grad.is_contiguous():
        raise ValueError("nti_adam_batched: param / m / v / grad must be [K, ...] of one shape, stats [K, 2], active [K]")
    if _is32(grad):
        _check(lib.ief_nti_adam_batched_f32g(param.data_ptr(), m.data_ptr(), v.data_ptr(), _act32(grad, "grad").data_ptr(),
                                             stats.data_ptr(), active.data_ptr(), hyper.data_ptr(), step.data_ptr(), total // K,
                                             K, _stream()), "ief_nti_adam_batched_f32g")
        return
    _dev16(grad, "grad"), _dev16(param16, "param16")
    if param16.numel() != total or not param16.is_contiguous():
        raise ValueError("nti_adam_batched: param16 shape mismatch")
    _check(lib.ief_nti_adam_batched_f32(param.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), stats.data_ptr(),
                                        active.data_ptr(), hyper.data_ptr(), step.data_ptr(), param16.data_ptr(), total // K, K,
                                        _stream()), "ief_nti_adam_batched_f32")
