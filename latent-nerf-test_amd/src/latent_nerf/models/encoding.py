"""Multiresolution hash-grid encoder (Instant-NGP), HIP-backed.  Counterpart of the `gridencoder`
extension of the absent src/latent_nerf/models/encoders; the level
table follows the align_corners=False convention recorded there."""
import ctypes
import math
import weakref
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from ..raymarching import backend as _b
from ..raymarching.raymarching import _chk, _p, _stream


class GridLevels:
    """Host-side level table shared with the kernels (offsets in rows, per-level scale, resolution)."""

    def __init__(self, num_levels=16, level_dim=2, base_resolution=16, desired_resolution=2048,
                 log2_hashmap_size=19, gridtype="hash"):
        if gridtype not in ("hash", "tiled", "blocked"):
            raise ValueError("gridtype must be 'hash' (Instant-NGP), 'tiled' (the upstream encoder's other layout: dense "
                             "index wrapped) or 'blocked' (4 x 2 x 2 vertex blocks per 64-byte line)")
        # flag OR-ed into the `variant` of every gather / scatter call (include/lnerf_hip.h LNERF_GRID_BLOCKED / _TILED)
        self.gridtype = gridtype
        self.flag = {"hash": 0, "blocked": _b.GRID_BLOCKED, "tiled": _b.GRID_TILED}[gridtype]
        if level_dim != 2:
            raise ValueError("only level_dim == 2 is built")
        if not (1 <= num_levels <= 32):
            raise ValueError("num_levels must be in [1, 32]")
        self.num_levels, self.level_dim = num_levels, level_dim
        self.base_resolution, self.desired_resolution = base_resolution, desired_resolution
        self.log2_hashmap_size = log2_hashmap_size
        max_params = 2 ** log2_hashmap_size
        pls = 2.0 ** (math.log2(desired_resolution / base_resolution) / (num_levels - 1)) if num_levels > 1 else 1.0
        S = math.log2(pls)
        offsets, scales, ress = [0], [], []
        for l in range(num_levels):
            res_host = int(math.ceil(base_resolution * pls ** l))
            n = min(max_params, (res_host + 1) ** 3)
            n = int(math.ceil(n / 8) * 8)
            offsets.append(offsets[-1] + n)
            scale = float(np.float32(2.0 ** (l * S) * base_resolution - 1.0))
            scales.append(scale)
            ress.append(int(math.ceil(scale)) + 1)
        self.offsets, self.scales, self.resolutions = offsets, scales, ress
        self.n_rows = offsets[-1]
        self.out_dim = num_levels * level_dim
        # ctypes views handed to the C ABI on every call
        self.c_offsets = (ctypes.c_int32 * (num_levels + 1))(*offsets)
        self.c_scales = (ctypes.c_float * num_levels)(*scales)
        self.c_res = (ctypes.c_int32 * num_levels)(*ress)


def _grid_args(levels: GridLevels, xyzs, bound, m_host, m_dev, level_stride, src, src_dtype=_b.F32):
    """The arguments every gather / scatter entry point starts with (src: the table of a gather, dfeat of a scatter)."""
    return (_chk(xyzs, "xyzs"), float(bound), src, src_dtype, levels.num_levels, levels.level_dim, levels.c_offsets,
            levels.c_scales, levels.c_res, int(m_host), _chk(m_dev, "m_dev", torch.int32, allow_none=True),
            int(level_stride))


def grid_encode_forward(xyzs, bound, table, levels: GridLevels, m_host, m_dev, level_stride, out=None,
                        out_dtype=torch.float32, variant=0):
    """xyzs [>=m_host,3] world positions -> level-major features [L, level_stride, 2]."""
    tdt = _b.F32 if table.dtype == torch.float32 else _b.BF16
    if table.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("table must be float32 or bfloat16")
    if out is None:
        out = torch.empty(levels.num_levels, level_stride, 2, device=xyzs.device, dtype=out_dtype)
    odt = _b.F32 if out.dtype == torch.float32 else _b.BF16
    _b.call("lnerf_grid_encode_forward", *_grid_args(levels, xyzs, bound, m_host, m_dev, level_stride,
                                                     _chk(table, "table", table.dtype), tdt),
            _chk(out, "feat", out.dtype), odt, int(variant) | levels.flag, _stream())
    return out


def grid_encode_backward_input(xyzs, bound, table, levels: GridLevels, dfeat, m_host, m_dev, level_stride, out=None):
    """Gradient of the features with respect to the sample positions (lnerf_grid_encode_backward_input): dfeat f32
    [L, level_stride, 2] level-major, `table` the table the forward read (f32 or bf16) -> dxyz [rows of xyzs, 3]; rows
    below min(m_host, *m_dev) are written, the others are zero (or keep what `out` held)."""
    if table.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("table must be float32 or bfloat16")
    tdt = _b.F32 if table.dtype == torch.float32 else _b.BF16
    if out is None:
        out = torch.zeros(xyzs.shape[0], 3, device=xyzs.device, dtype=torch.float32)
    _b.call("lnerf_grid_encode_backward_input", *_grid_args(levels, xyzs, bound, m_host, m_dev, level_stride,
                                                            _chk(table, "table", table.dtype), tdt),
            _chk(dfeat, "dfeat"), _chk(out, "dxyz"), levels.flag, _stream())
    return out


_scatter_ws = {}   # device -> [workspaces, ascending size]


def scatter_workspace(levels: GridLevels, m_host, device):
    """Device scratch of the bucketed scatter: ANY buffer of at least lnerf_grid_encode_backward_workspace_bytes()
    serves (the kernels lay it out from `m_host`, not from its size), so a process keeps one buffer per device that only
    ever grows: a renderer whose sample budget moves up and down in 64 Ki steps (NeRFRenderer.update_sample_budget)
    re-uses the largest one instead of allocating one per distinct capacity.  A captured hipGraph may hold the address
    of a buffer handed out earlier, so outgrown ones are kept, but every growth is by >= 1.5x: the total stays below
    three times the largest request."""
    need = _b.get_lib().lnerf_grid_encode_backward_workspace_bytes(levels.num_levels, levels.c_offsets, int(m_host))
    if need == 0:
        raise _b.LnerfError("bucketed scatter cannot handle this level table; use scatter variant 0/1")
    have = _scatter_ws.setdefault(str(device), [])
    for ws in have:
        if ws.numel() >= need:
            return ws
    size = max(need, (3 * have[-1].numel()) // 2 if have else 0)
    ws = torch.empty(size, device=device, dtype=torch.uint8)
    # header: level maxima and arrival counters start out clean (LNERF_SCATTER_ZERO_HEAD_BYTES; the calls keep them so)
    ws[:min(size, _b.SCATTER_ZERO_HEAD_BYTES)].zero_()
    have.append(ws)
    return ws


# Whether the level maxima at the head of a device's (shared) scatter workspace are known to be ZERO, and a counter of the
# scatter calls issued through it from Python.  The workspace is one buffer per DEVICE, so this is tracked per device, not
# per encoder: a second model -- or a backward through the same net outside the training step -- leaves its maxima in the
# header, and a step that passes LNERF_SCATTER_CLEARED on the strength of its OWN previous call would scale with stale,
# larger maxima (no overflow, but fixed-point precision drops and graph == eager is lost).  A captured hipGraph bakes the
# flag in: whoever replays one compares scatter_workspace_epoch() with the value it noted at capture time and captures
# again when a foreign call went through in between (Trainer.train()).
_ws_state = {}   # str(device) -> [data_ptr of the workspace whose maxima are zero | None, epoch]


def _ws(device):
    return _ws_state.setdefault(str(device), [None, 0])


def ws_mark_dirty(device):
    st = _ws(device)
    st[0], st[1] = None, st[1] + 1


def ws_mark_clean(wst):
    st = _ws(wst.device)
    st[0], st[1] = wst.data_ptr(), st[1] + 1


def ws_is_clean(wst):
    return _ws(wst.device)[0] == wst.data_ptr()


def scatter_workspace_epoch(device):
    """(clean workspace pointer, number of scatter calls issued from Python on this device): changes whenever anybody
    scatters through the device's workspace outside a graph replay."""
    return tuple(_ws(device))


_clear_bytes = {}


def scatter_clear_bytes(levels: GridLevels, m_host):
    """Bytes at the head of the scatter workspace that a call clears (lnerf_grid_scatter_clear_bytes); a caller that
    zeroes them itself passes `variant | backend.SCATTER_CLEARED`."""
    key = (tuple(levels.offsets), int(m_host))
    n = _clear_bytes.get(key)
    if n is None:
        n = int(_b.get_lib().lnerf_grid_scatter_clear_bytes(levels.num_levels, levels.c_offsets, int(m_host)))
        _clear_bytes[key] = n
    return n


def grid_encode_backward(xyzs, bound, dfeat, levels: GridLevels, m_host, m_dev, level_stride, dtable, variant=2):
    """dtable (f32 [rows,2]) += scatter of dfeat (level-major, f32).
    variant 0/1: global float atomics; 2: two-pass bucketed scatter (LDS reduction); 3: the same with packed
    8-byte records (values rounded to 17 mantissa bits)."""
    ws, ws_bytes = None, 0
    if (variant & 0xFF) >= 2:
        wst = scatter_workspace(levels, m_host, xyzs.device)
        ws, ws_bytes = _p(wst), wst.numel()
        ws_mark_dirty(xyzs.device)      # (this call leaves its level maxima in the shared workspace)
    _b.call("lnerf_grid_encode_backward", *_grid_args(levels, xyzs, bound, m_host, m_dev, level_stride,
                                                      _chk(dfeat, "dfeat")),
            _chk(dtable, "dtable"), int(variant) | levels.flag, ws, ws_bytes, _stream())
    return dtable


def grid_tv_plan(levels: GridLevels, tv_vertices=65536):
    """Line plan of the total-variation term (lnerf_grid_tv_plan, host only): [L + 1] line offsets, level l takes
    min((res_l + 1)^2, max(1, tv_vertices // (res_l + 1))) whole x-lines of its vertex lattice per step."""
    out = (ctypes.c_int32 * (levels.num_levels + 1))()
    _b.call("lnerf_grid_tv_plan", levels.num_levels, levels.c_res, int(tv_vertices), out)
    return list(out)


def grid_tv_lines(levels: GridLevels, plan, seed=0, step=0, step_dev=None, device=None, out=None):
    """The (y, z) of every line of `plan` (grid_tv_plan) at (seed, step) -- `step_dev` (device int32) replaces `step`
    when given -- as int32 [plan[-1], 2] (lnerf_grid_tv_lines)."""
    if out is None:
        if device is None:
            raise ValueError("grid_tv_lines: give `device` or `out`")
        if torch.device(device).type != "cuda":
            raise ValueError("grid_tv_lines: lines must live on the GPU (got %s); there is no CPU path" % (device,))
        out = torch.empty(plan[-1], 2, device=device, dtype=torch.int32)
    if tuple(out.shape) != (plan[-1], 2):
        raise ValueError("grid_tv_lines: lines must be [%d, 2]" % plan[-1])
    c_plan = (ctypes.c_int32 * len(plan))(*plan)
    _b.call("lnerf_grid_tv_lines", levels.num_levels, levels.c_res, c_plan, int(seed) & 0xFFFFFFFF,
            int(step) & 0xFFFFFFFF, _chk(step_dev, "step_dev", torch.int32, allow_none=True),
            _chk(out, "lines", torch.int32), _stream())
    return out


def grid_tv_grad(table, levels: GridLevels, plan, weights, dtable, lines=None, seed=0, step=0, step_dev=None):
    """dtable (f32 [rows, 2]) += the total-variation term of `table` (the f32 master) on the lines of `plan`
    (lnerf_grid_tv_grad; see include/lnerf_hip.h): weights[l] per sampled vertex of level l, 0 skips the level; `lines`
    int32 [plan[-1], 2] or None = drawn inside the launch from (seed, step | *step_dev)."""
    if len(weights) != levels.num_levels or len(plan) != levels.num_levels + 1:
        raise ValueError("grid_tv_grad: need one weight per level and L + 1 line offsets")
    if tuple(table.shape) != (levels.n_rows, 2) or tuple(dtable.shape) != (levels.n_rows, 2):
        raise ValueError("grid_tv_grad: table and dtable must be [%d, 2]" % levels.n_rows)
    if lines is not None and tuple(lines.shape) != (plan[-1], 2):
        raise ValueError("grid_tv_grad: lines must be [%d, 2]" % plan[-1])
    c_plan = (ctypes.c_int32 * len(plan))(*plan)
    c_w = (ctypes.c_float * levels.num_levels)(*[float(w) for w in weights])
    _b.call("lnerf_grid_tv_grad", _chk(table, "table"), levels.num_levels, levels.level_dim, levels.c_offsets, levels.c_res,
            levels.flag, c_plan, _chk(lines, "lines", torch.int32, allow_none=True), int(seed) & 0xFFFFFFFF,
            int(step) & 0xFFFFFFFF, _chk(step_dev, "step_dev", torch.int32, allow_none=True), c_w, _chk(dtable, "dtable"),
            _stream())
    return dtable


class FusedTableUpdate:
    """Set on a GridEncoder (`encoder.fused_update`) by FusedAdam(fuse_table_update=True).  When ARMED
    (FusedAdam.arm(), once per step, right before the step's single backward) the scatter of that backward applies
    the table's Adam step itself (lnerf_grid_encode_backward_adam) and the table gets no `.grad`; any other
    backward through the encoder (unarmed) produces the ordinary gradient.  Single GPU only."""

    def __init__(self, exp_avg, exp_avg_sq, lr, betas, eps, optimizer, levels=None):
        self.exp_avg, self.exp_avg_sq = exp_avg, exp_avg_sq
        # the MOMENT MAP (include/lnerf_hip.h, lnerf_moment_map_*): one byte per 16-row group, non-zero where a moment has
        # a non-zero bit; the fused step leaves clean groups without gradient alone and keeps the map current.  Owned
        # here, bound to exp_avg in the library for as long as this object lives, never part of a state_dict.  Whatever
        # else writes the moments calls rebuild_map() on the same stream (FusedAdam does).
        self.levels, self.map = levels, None
        if levels is not None and exp_avg.is_cuda:
            n = int(_b.get_lib().lnerf_moment_map_bytes(levels.num_levels, levels.c_offsets))
            if n == 0:
                raise _b.LnerfError("lnerf_moment_map_bytes: this level table has no bucket plan")
            self.map = torch.empty(n, device=exp_avg.device, dtype=torch.uint8)
            self.rebuild_map()
            _b.call("lnerf_moment_map_bind", _p(exp_avg), _p(self.map), n)
            # (by pointer value: the finalizer must not keep the tensors alive; they outlive it through self)
            weakref.finalize(self, _unbind_moment_map, exp_avg.data_ptr()).atexit = False
        self.lr, self.betas, self.eps = float(lr), betas, float(eps)
        self.optimizer = optimizer          # step number / device step counter live there
        self.zero = torch.zeros_like(exp_avg)  # dtable scratch argument of the fused entry points (never written)
        self.applied = 0                    # fused updates since the last optimizer.step()
        self.armed = False
        # tail mode (FusedAdam(tail=True)): the armed backward leaves the sum of the MLP's gradient slabs to ONE launch
        # in optimizer.step() (lnerf_step_tail), which also steps the MLP's parameters, ticks the step counter and
        # leaves the scatter's level maxima zero for the next step
        self.tail = False
        self.pending_tail = None            # (levels, m_host, variant, scatter workspace, mlp workspace, precision, out_dim)
        # the armed backward closed the step itself (grid_encode_backward_adam_tail): slab sums, the MLP's Adam step, the
        # tick of the step counter all ran inside the scatter's pass 2
        self.closed = False
        self.inline_tail = False            # set by FusedAdam: the tail may run inside the scatter (no other small parameter)

    def rebuild_map(self):
        """The moment map from the moments as they are (one streaming launch on the current stream): call behind anything
        but the fused step that wrote exp_avg / exp_avg_sq, before the next armed backward."""
        if self.map is not None:
            lv = self.levels
            _b.call("lnerf_moment_map_build", _p(self.exp_avg), _p(self.exp_avg_sq), lv.num_levels, lv.level_dim,
                    lv.c_offsets, _p(self.map), self.map.numel(), _stream())


def _unbind_moment_map(exp_avg_ptr):
    try:
        _b.get_lib().lnerf_moment_map_bind(ctypes.c_void_p(exp_avg_ptr), None, 0)
    except Exception:   # (interpreter shutdown: the library may be gone)
        pass


def grid_encode_backward_adam(xyzs, bound, dfeat, encoder, m_host, m_dev, level_stride, variant):
    """Scatter of dfeat fused with the Adam step of encoder.embeddings (see include/lnerf_hip.h)."""
    fu = encoder.fused_update
    levels = encoder.levels
    if (variant & 0xFF) < 2:
        raise _b.LnerfError("the fused table update needs the bucketed scatter (variant 2 or 3)")
    wst = scatter_workspace(levels, m_host, xyzs.device)
    opt = fu.optimizer
    b1, b2 = fu.betas
    _b.call("lnerf_grid_encode_backward_adam", *_grid_args(levels, xyzs, bound, m_host, m_dev, level_stride,
                                                           _chk(dfeat, "dfeat")),
            _p(fu.zero), int(variant) | levels.flag, _p(wst), wst.numel(), _p(encoder.embeddings.data), _p(fu.exp_avg),
            _p(fu.exp_avg_sq), _p(encoder.shadow()), fu.lr, b1, b2, fu.eps, opt.step_no + 1, _p(opt.step_dev),
            float(opt.grad_scale), _stream())
    ws_mark_dirty(xyzs.device)


def grid_encode_backward_adam_tail(xyzs, bound, dfeat, encoder, m_host, m_dev, level_stride, variant, mlp_ws, precision,
                                   out_dim):
    """The armed scatter that also CLOSES the step (lnerf_grid_encode_backward_adam_tail): the workgroups of its pass 2
    sum the MLP's gradient slabs, step the MLP's six tensors, advance the device step counter and leave the level maxima
    zero for the next step -- no launch behind the scatter.  FusedAdam(tail=True) with no other small parameter."""
    fu = encoder.fused_update
    levels = encoder.levels
    opt = fu.optimizer
    t = opt.tail_args()
    wst = scatter_workspace(levels, m_host, xyzs.device)
    b1, b2 = fu.betas
    _b.call("lnerf_grid_encode_backward_adam_tail", *_grid_args(levels, xyzs, bound, m_host, m_dev, level_stride,
                                                                _chk(dfeat, "dfeat")),
            _p(fu.zero), int(variant) | levels.flag, _p(wst), wst.numel(), _p(encoder.embeddings.data), _p(fu.exp_avg),
            _p(fu.exp_avg_sq), _p(encoder.shadow()), fu.lr, _p(mlp_ws), mlp_ws.numel(), int(precision), int(out_dim),
            t["p"], t["m"], t["v"], float(t["lr"]), t["maps"], b1, b2, fu.eps, opt.step_no + 1, _p(opt.step_dev),
            float(opt.grad_scale), _b.TAIL_TICK | _b.TAIL_CLEAR_SCATTER, _stream())
    ws_mark_clean(wst)               # (level maxima zero again when the launch ends)


class GradSink:
    """Set on a GridEncoder (`encoder.grad_sink`) by GradSync.attach_sink(): the backward pass WRITES the table
    gradient as bf16 into `wire` (lnerf_grid_encode_backward_bf16) -- the buffer the data-parallel all-reduce sends --
    instead of accumulating an f32 `.grad`: no zero fill, no read-modify-write, no cast.  One backward per step.

    `groups` (list of (level_lo, level_hi)) selects the PIPELINED form: the backward pass only bins the records
    (lnerf_grid_scatter_bin); GradSync.allreduce_pipelined() then sums one level group at a time
    (lnerf_grid_scatter_reduce_bf16) and launches that group's all-reduce while the next group is being summed."""

    def __init__(self, table, groups=None):
        self.wire = torch.zeros(table.shape, device=table.device, dtype=torch.bfloat16)
        self.zero = torch.zeros(table.shape, device=table.device, dtype=torch.float32)  # overflow records only
        self.groups = groups
        self.pending = None   # (bound, levels, m_host, level_stride, variant, workspace) of a binned, not yet summed backward
        # {data_ptr of a small parameter: its view of GradSync's flat bucket}: a backward pass may write such a gradient
        # there directly (and sets small_written, for good: replays of a captured backward repeat the write without any
        # Python); None: everything goes through `.grad`
        self.small_direct = None
        self.small_written = False
        self.shard_ranges, self.shard_rest = None, None   # row-sharded optimiser (GradSync._plan_shards)


def level_groups(levels: GridLevels, n_groups=4):
    """Level ranges of roughly equal table rows (the exchange is priced per row): [(lo, hi), ...]."""
    n_groups = max(1, min(int(n_groups), levels.num_levels))
    target = levels.n_rows / n_groups
    out, lo = [], 0
    for l in range(levels.num_levels):
        done_rows = levels.offsets[l + 1]
        if done_rows >= target * (len(out) + 1) - 1e-9 or l == levels.num_levels - 1:
            if len(out) < n_groups - 1 or l == levels.num_levels - 1:
                out.append((lo, l + 1))
                lo = l + 1
    if lo < levels.num_levels:
        out.append((lo, levels.num_levels))
    return out


def grid_encode_backward_bf16(xyzs, bound, dfeat, encoder, m_host, m_dev, level_stride, variant, binned=False):
    """encoder.grad_sink.wire = the table gradient in bf16 (written, not accumulated).  binned: pass 1 only
    (lnerf_grid_scatter_bin), grid_scatter_reduce_group sums the records later.  Returns the scatter workspace."""
    sink = encoder.grad_sink
    levels = encoder.levels
    if variant < 2:
        raise _b.LnerfError("the bf16 gradient output needs the bucketed scatter (variant 2 or 3)")
    wst = scatter_workspace(levels, m_host, xyzs.device)
    ws_mark_dirty(xyzs.device)
    args = (*_grid_args(levels, xyzs, bound, m_host, m_dev, level_stride, _chk(dfeat, "dfeat")), _p(sink.zero),
            int(variant) | levels.flag, _p(wst), wst.numel())
    if binned:
        _b.call("lnerf_grid_scatter_bin", *args, _stream())
    else:
        _b.call("lnerf_grid_encode_backward_bf16", *args, _p(sink.wire), _stream())
    return wst


def grid_scatter_reduce_group(sink: GradSink, level_lo, level_hi):
    """Pass 2 of levels [level_lo, level_hi) of the backward that sink.pending describes: writes rows
    offsets[level_lo] .. offsets[level_hi] of sink.wire."""
    if sink.pending is None:
        raise _b.LnerfError("no binned backward pass is pending on this gradient sink")
    bound, levels, m_host, level_stride, variant, wst = sink.pending
    _b.call("lnerf_grid_scatter_reduce_bf16", bound, levels.num_levels, levels.level_dim, levels.c_offsets,
            levels.c_scales, levels.c_res, m_host, level_stride, int(level_lo), int(level_hi), _p(sink.zero), variant,
            _p(wst), wst.numel(), _p(sink.wire), _stream())


class Route(NamedTuple):
    """What one backward through the encoder does with the table gradient (`name`), and what the fused MLP launch in
    front of its scatter owes for it -- see backward_route:
      plain              lnerf_grid_encode_backward into a fresh f32 gradient of the table
      wire               lnerf_grid_encode_backward_bf16 into GradSink.wire (data parallel, bf16 on the wire)
      bin                lnerf_grid_scatter_bin; pass 2 follows per level group in GradSync.allreduce_pipelined()
      adam               lnerf_grid_encode_backward_adam: the table's Adam step inside the scatter (FusedAdam.arm())
      adam_tail          the same; FusedAdam.step() closes the step (lnerf_step_tail)
      adam_closing_tail  lnerf_grid_encode_backward_adam_tail: the scatter's pass 2 closes the step itself
    On a tail route the MLP launch writes no weight gradient: the step's tail sums its gradient slabs."""
    name: str
    variant: int                          # the scatter's variant, SCATTER_CLEARED included
    clear: bool = False                   # the MLP launch clears the scatter's cursors on the side
    views: Optional[list] = None          # ... and writes its weight gradients into these views of the exchange bucket
    ws: Optional[torch.Tensor] = None     # the scatter workspace (plan_backward)

    @property
    def tail(self):
        return self.name in ("adam_tail", "adam_closing_tail")

    def mlp_args(self, levels: GridLevels, m_host):
        """(flags OR-ed into the MLP backward's precision tag, clear_ptr, clear_bytes)."""
        clear = (_p(self.ws), scatter_clear_bytes(levels, m_host)) if self.clear else (None, 0)
        return (_b.MLP_DEFER_REDUCE if self.tail else 0,) + clear


def backward_route(fu, sink, variant, m_host, mlp=None, own_ws=False, ws_clean=False):
    """The Route of one backward through an encoder (reads its arguments, changes nothing).  fu, sink: the encoder's
    FusedTableUpdate and GradSink or None; variant: its scatter variant; mlp: the six tensors of the fused MLP node whose
    launch precedes the scatter (None: the bare encoder); own_ws: that launch runs in the node's own workspace (the tail
    reads the gradient slabs there); ws_clean: the scatter workspace's level maxima are zero (ws_is_clean)."""
    bucketed = variant >= 2 and m_host > 0
    armed = fu is not None and fu.armed
    if armed and fu.tail and mlp is not None and own_ws and bucketed:
        return Route("adam_closing_tail" if fu.inline_tail else "adam_tail",
                     variant | (_b.SCATTER_CLEARED if ws_clean else 0))
    clear = mlp is not None and bucketed       # (one dispatch less per step than the scatter's own fill)
    views = None
    if mlp is not None and sink is not None and sink.groups and sink.small_direct:
        # pipelined exchange: no `.grad`, no pack copy into the flat bucket the all-reduce sends (one dispatch less)
        found = [sink.small_direct.get(t.data_ptr()) for t in mlp]
        if all(v is not None and v.shape == t.shape for v, t in zip(found, mlp)):
            views = found
    name = "adam" if armed else "plain" if sink is None else "bin" if sink.groups else "wire"
    return Route(name, variant | (_b.SCATTER_CLEARED if clear else 0), clear, views)


def plan_backward(encoder, m_host, device, mlp=None, own_ws=False):
    """backward_route() of a backward through `encoder` now (arguments as there), with the scatter workspace."""
    sv = encoder.scatter_variant
    ws = scatter_workspace(encoder.levels, m_host, device) if (mlp is not None and sv >= 2 and m_host > 0) else None
    return backward_route(encoder.fused_update, encoder.grad_sink, sv, m_host, mlp, own_ws,
                          ws is not None and ws_is_clean(ws))._replace(ws=ws)


def run_backward(route, xyzs, bound, dfeat, encoder, m_host, m_dev, level_stride, mlp_ws=None, precision=0, out_dim=0):
    """Issues the scatter of a planned `route` and the bookkeeping it owes (each scatter call marks the shared workspace
    itself); mlp_ws, precision, out_dim: the fused MLP's, for the tail.  -> the f32 table gradient of the plain route."""
    fu, sink, levels = encoder.fused_update, encoder.grad_sink, encoder.levels
    args = (xyzs, bound, dfeat, encoder, m_host, m_dev, level_stride, route.variant)
    if route.name == "plain":
        return grid_encode_backward(xyzs, bound, dfeat, levels, m_host, m_dev, level_stride,
                                    torch.zeros(encoder.embeddings.shape, device=xyzs.device), route.variant)
    if route.name == "wire":
        grid_encode_backward_bf16(*args)
    elif route.name == "bin":
        # (`pending` stays after the exchange: a replayed hipGraph bins again without running any Python)
        sink.pending = (float(bound), levels, int(m_host), int(level_stride), int(route.variant),
                        grid_encode_backward_bf16(*args, binned=True))
    else:
        fu.armed = False
        if route.name == "adam_closing_tail":
            grid_encode_backward_adam_tail(*args, mlp_ws, precision, out_dim)
            fu.closed = True         # optimizer.step() has nothing left to launch
        else:
            grid_encode_backward_adam(*args)
            if route.name == "adam_tail":
                fu.pending_tail = (levels, int(m_host), int(encoder.scatter_variant), route.ws, mlp_ws, int(precision),
                                   int(out_dim))
        fu.applied += 1
    if route.views is not None:
        sink.small_written = True


class _GridEncode(torch.autograd.Function):
    """feat = encode(xyzs; table).  `table` is the f32 master parameter (gradient target);
    `shadow` an optional bf16 copy that the gather actually reads."""

    @staticmethod
    def forward(ctx, xyzs, table, shadow, encoder, bound, m_host, m_dev, level_stride, feat_dtype):
        src = table if shadow is None else shadow
        feat = grid_encode_forward(xyzs, bound, src.detach(), encoder.levels, m_host, m_dev, level_stride, None,
                                   feat_dtype, encoder.variant)
        ctx.save_for_backward(xyzs, m_dev if m_dev is not None else torch.empty(0))
        ctx.meta = (encoder, bound, m_host, m_dev is not None, level_stride)
        # the position gradient reads the table the gather read (the bf16 shadow where there is one)
        ctx.src = src.detach() if ctx.needs_input_grad[0] else None
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        xyzs, m_dev = ctx.saved_tensors
        encoder, bound, m_host, has_mdev, level_stride = ctx.meta
        dfeat = dfeat.contiguous().float()
        route = plan_backward(encoder, m_host, xyzs.device)
        dtable = run_backward(route, xyzs, bound, dfeat, encoder, m_host, m_dev if has_mdev else None, level_stride)
        dxyz = None
        if ctx.needs_input_grad[0]:
            dxyz = grid_encode_backward_input(xyzs, bound, ctx.src, encoder.levels, dfeat, m_host,
                                              m_dev if has_mdev else None, level_stride)
        return dxyz, dtable, None, None, None, None, None, None, None


class GridEncoder(nn.Module):
    """embeddings: f32 [n_rows, 2] master table (U(-1e-4, 1e-4) init).  With
    `table_dtype=torch.bfloat16` the gather reads a bf16 shadow that is refreshed lazily whenever
    the master changed (or explicitly by the fused Adam step)."""

    def __init__(self, num_levels=16, level_dim=2, base_resolution=16, desired_resolution=2048,
                 log2_hashmap_size=19, table_dtype=torch.float32, variant=0, scatter_variant=2, gridtype="hash"):
        super().__init__()
        self.levels = GridLevels(num_levels, level_dim, base_resolution, desired_resolution, log2_hashmap_size,
                                 gridtype=gridtype)
        self.out_dim = self.levels.out_dim
        self.variant = variant
        self.scatter_variant = scatter_variant
        self.table_dtype = table_dtype
        self.embeddings = nn.Parameter(torch.empty(self.levels.n_rows, level_dim))
        self.reset_parameters()
        self._shadow = None
        self._shadow_version = -1
        self.fused_update = None  # FusedTableUpdate, installed by FusedAdam(fuse_table_update=True)
        self.grad_sink = None     # GradSink, installed by GradSync.attach_sink() (data parallel, bf16 on the wire)
        self._tv_plans = {}       # tv_vertices -> (line offsets, sampled vertices per level) of grad_total_variation

    def reset_parameters(self):
        self.embeddings.data.uniform_(-1e-4, 1e-4)

    def shadow(self):
        if self.table_dtype == torch.float32:
            return None
        ver = self.embeddings._version
        if self._shadow is None or self._shadow.device != self.embeddings.device:
            self._shadow = torch.empty(self.levels.n_rows, 2, device=self.embeddings.device, dtype=torch.bfloat16)
            self._shadow_version = -1
        if self._shadow_version != ver:
            _b.call("lnerf_cast_f32_to_bf16", _p(self.embeddings.data), _p(self._shadow),
                    self.embeddings.numel(), _stream())
            self._shadow_version = ver
        return self._shadow

    def mark_shadow_fresh(self):
        """Called by the fused optimiser step, which rewrites the shadow in the same pass."""
        self._shadow_version = self.embeddings._version

    def grad_total_variation(self, weight, tv_vertices=65536, seed=0, step=None, step_dev=None, grad=None, lines=None):
        """Adds the gradient of the table's total-variation regulariser (the upstream encoder's `grad_total_variation`,
        the trainers' `lambda_tv`) into `grad` (default: `embeddings.grad`, which must exist): per level, `weight` / n_l
        times the sum of the differences to the axis neighbours on n_l sampled lattice vertices -- whole x-lines, drawn
        from (seed, step), or from (seed, *step_dev) when the optimiser's device counter is given; coarse levels are swept
        whole.  One launch (lnerf_grid_tv_grad); reads the f32 master, leaves table and shadow alone.  `lines`: explicit
        int32 [grid_tv_plan(...)[-1], 2] lines instead of drawn ones."""
        if grad is None:
            grad = self.embeddings.grad
            if grad is None:
                raise RuntimeError("grad_total_variation: embeddings.grad does not exist (call it after backward(), or "
                                   "pass `grad`)")
        key = int(tv_vertices)
        plan = self._tv_plans.get(key)
        if plan is None:
            plan = grid_tv_plan(self.levels, key)
            res = self.levels.resolutions
            self._tv_plans[key] = plan = (plan, [(plan[l + 1] - plan[l]) * (res[l] + 1) for l in range(len(res))])
        plan, n_vertices = plan
        weights = [float(weight) / n for n in n_vertices]
        if step is None:
            step = 0
        return grid_tv_grad(self.embeddings.data, self.levels, plan, weights, grad, lines, seed, step, step_dev)

    def encode(self, xyzs, bound, m_host, m_dev=None, level_stride=None, feat_dtype=torch.float32):
        """Level-major features [L, level_stride, 2] (differentiable w.r.t. embeddings, and w.r.t. xyzs when it
        requires grad: first order only)."""
        if level_stride is None:
            level_stride = xyzs.shape[0]
        return _GridEncode.apply(xyzs, self.embeddings, self.shadow(), self, bound, m_host, m_dev, level_stride,
                                 feat_dtype)

    def forward(self, inputs, bound=1.0):
        """inputs [..., 3] in [-bound, bound] -> [..., L*2] (sample-major view, as the upstream encoder)."""
        prefix = inputs.shape[:-1]
        x = inputs.reshape(-1, 3).contiguous().float()
        M = x.shape[0]
        feat = self.encode(x, bound, M)
        return feat.permute(1, 0, 2).reshape(*prefix, self.out_dim)
