"""Float64 / exact-integer restatement of the hash table's total-variation term (csrc/grid_tv.hip, include/lnerf_hip.h
lnerf_grid_tv_plan / _lines / _grad, GridEncoder.grad_total_variation).  Not a test file.

Level l has the vertex lattice [0, res_l]^3; row_l(p) is oracle.nerf_oracle.grid_corner_indices (it takes vertex
coordinates directly); e(p) = table[offsets[l] + row_l(p)].  For every sampled vertex p and channel c
    g[offsets[l] + row_l(p), c] += w_l * sum over q in N(p) of (e_c(p) - e_c(q))
with N(p) the up to six axis neighbours inside the lattice.  `energy` is the function this is the gradient of when every
vertex is sampled with w_l = lam / N_l:  R_l = lam / (2 N_l) * sum over lattice edges |e(p) - e(q)|^2."""
import numpy as np
import torch

from oracle import nerf_oracle as O

LAYOUTS = ("hash", "blocked", "tiled")


def levels(layout, num_levels=5, base=4, desired=96, log2_T=12):
    """The five-level table of the tests: res [4, 9, 20, 44, 96], rows [128, 1000, 4096, 4096, 4096] -- two dense and
    three hashed levels, 97-vertex lines on the last one."""
    return O.make_grid_levels(num_levels, 2, base, desired, log2_T, blocked=layout == "blocked", tiled=layout == "tiled")


def plan(resolutions, tv_vertices):
    """[L + 1] line offsets: level l takes min((res + 1)^2, max(1, tv_vertices // (res + 1))) lines."""
    out = [0]
    for res in resolutions:
        s = res + 1
        out.append(out[-1] + min(s * s, max(1, int(tv_vertices) // s)))
    return out


def full_plan(resolutions):
    out = [0]
    for res in resolutions:
        out.append(out[-1] + (res + 1) ** 2)
    return out


def draw_lines(resolutions, offs, seed, step):
    """int64 [offs[-1], 2] = (y, z) of every line, exact integers: a level whose plan takes every line is swept in plane
    order; otherwise line j comes from stratum j: lo_j = j S // n, idx = lo_j + h mod (lo_{j+1} - lo_j), h = the
    counter_hash (csrc/common.h; O.occ_hash) of (j, seed, step, level)."""
    out = np.zeros((offs[-1], 2), dtype=np.int64)
    for l, res in enumerate(resolutions):
        s, n = res + 1, offs[l + 1] - offs[l]
        S = s * s
        assert 1 <= n <= S and n * S < 2 ** 62
        j = np.arange(n, dtype=np.uint64)
        if n == S:
            idx = j
        else:
            lo = j * np.uint64(S) // np.uint64(n)
            hi = (j + np.uint64(1)) * np.uint64(S) // np.uint64(n)
            assert (hi > lo).all()
            h = O.occ_hash(j, int(seed), int(step), l)
            idx = lo + h % (hi - lo)
        idx = idx.astype(np.int64)
        out[offs[l]:offs[l + 1], 0] = idx % s
        out[offs[l]:offs[l + 1], 1] = idx // s
    return out


def all_lines(resolutions):
    """The lines of full_plan(): every (y, z) of every level, plane order."""
    return draw_lines(resolutions, full_plan(resolutions), 0, 0)


def _rows(lv, l, pts):
    hs = lv.offsets[l + 1] - lv.offsets[l]
    return O.grid_corner_indices(pts, lv.resolutions[l], hs, blocked=lv.blocked, tiled=lv.tiled)


def line_vertices(res, yz):
    """yz int64 [n, 2] -> lattice points int64 [n * (res + 1), 3] (x fastest)."""
    yz = torch.as_tensor(yz, dtype=torch.int64)
    n, s = yz.shape[0], res + 1
    x = torch.arange(s, dtype=torch.int64).repeat(n)
    return torch.stack([x, yz[:, 0].repeat_interleave(s), yz[:, 1].repeat_interleave(s)], dim=-1)


def sampled_rows(lv, offs, lines):
    """Sorted unique global rows of the sampled vertices of all levels (int64 tensor)."""
    out = []
    for l, res in enumerate(lv.resolutions):
        pts = line_vertices(res, lines[offs[l]:offs[l + 1]])
        out.append(_rows(lv, l, pts) + lv.offsets[l])
    return torch.unique(torch.cat(out))


def tv_grad(table, lv, offs, lines, weights, initial=None):
    """-> (g, A, k), float64 [rows, 2], float64 [rows, 2], int64 [rows]:  g = initial + the term;  A = |initial| + w *
    sum over the row's contributions of sum over q of (|e_p| + |e_q|), per channel: the magnitude every rounding of the
    f32 evaluation is relative to;  k = contributions the row collects (levels with weight 0 contribute nothing)."""
    e_all = torch.as_tensor(table).double()
    g = torch.zeros_like(e_all) if initial is None else torch.as_tensor(initial).double().clone()
    A = g.abs()
    k = torch.zeros(e_all.shape[0], dtype=torch.int64)
    for l, res in enumerate(lv.resolutions):
        w = float(weights[l])
        if w == 0.0:
            continue
        e = e_all[lv.offsets[l]:lv.offsets[l + 1]]
        pts = line_vertices(res, lines[offs[l]:offs[l + 1]])
        rp = _rows(lv, l, pts)
        ep = e[rp]
        acc, mag = torch.zeros_like(ep), torch.zeros_like(ep)
        for axis in range(3):
            for d in (-1, 1):
                q = pts.clone()
                q[:, axis] += d
                ok = ((q[:, axis] >= 0) & (q[:, axis] <= res))[:, None].double()
                q[:, axis].clamp_(0, res)
                eq = e[_rows(lv, l, q)]
                acc += ok * (ep - eq)
                mag += ok * (ep.abs() + eq.abs())
        rows = rp + lv.offsets[l]
        g.index_add_(0, rows, w * acc)
        A.index_add_(0, rows, abs(w) * mag)
        k += torch.bincount(rows, minlength=k.shape[0])
    return g, A, k


def energy(table, lv, lam=1.0):
    """sum over the levels of lam / (2 N_l) * sum over lattice edges |e(p) - e(q)|^2 (differentiable, any dtype)."""
    total = table.new_zeros(())
    for l, res in enumerate(lv.resolutions):
        s = res + 1
        ax = torch.arange(s, dtype=torch.int64)
        zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
        pts = torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3)
        e = table[lv.offsets[l]:lv.offsets[l + 1]][_rows(lv, l, pts)].reshape(s, s, s, -1)   # [z, y, x, c]
        edges = ((e[1:] - e[:-1]) ** 2).sum() + ((e[:, 1:] - e[:, :-1]) ** 2).sum() + ((e[:, :, 1:] - e[:, :, :-1]) ** 2).sum()
        total = total + lam / (2.0 * s ** 3) * edges
    return total
