"""The float64 lattice-point reference of the training march (tests/march_reference.py) on the CPU: the oracle's march
passes it on every case, and the checker rejects every perturbation of the oracle's output, naming the rule."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import march_reference as R


@pytest.mark.parametrize("name", R.case_names())
def test_oracle_march_passes_the_reference(name):
    case, out = R.build_case(name), R.oracle_march(name)
    st = R.assert_case(name, out)
    s = case.ref.stats
    print("%-28s rays %3d lattice %7d free %6.3f%% must %6.2f%% of occupied; samples %6d, on free points %d" % (
        name, case.ro.shape[0], s["lattice"], 100 * s["free_share"], 100 * s["must_share"], st["samples"], st["on_free"]))
    assert st["samples"] == int(out.rays[:, 2].sum()) > 0
    # the defined misses have no samples
    for e in ("inface", "miss", "near_past_far"):
        assert int(out.rays[case.edge[e], 2]) == 0, e


def test_case_table():
    """The free-share table of the module docstring: per configuration the largest free share and the smallest must
    share over its cases (pytest -s prints it)."""
    for cname in R.CONFIGS:
        st = [R.build_case(n).ref.stats for n in R.case_names() if n.split("-")[0] == cname]
        free, must = max(s["free_share"] for s in st), min(s["must_share"] for s in st)
        print("    %-11s %-28s free <= %.2f %%   must >= %.1f %%" % (cname, R.CONFIGS[cname], 100 * free, 100 * must))
        assert free <= 0.03 and must >= 0.90


def test_the_inverted_cases_step_by_dt_max():
    """dt_min > dt_max: the one step rule yields dt_max, at dt_gamma = 0 as well."""
    for cname in ("inverted16", "inverted64"):
        bound, cascade, G, max_steps, dt_gamma = R.CONFIGS[cname]
        dt_min, dt_max = R.step_constants(cascade, G, max_steps)
        assert dt_min > dt_max and dt_gamma == 0.0
        out = R.oracle_march(cname + "-full")
        assert bool((out.deltas[:, 0] == np.float32(dt_max)).all())


# ---------------------------------------------------------------------------------------------- perturbations
def _rows(out):
    """Per-ray [count, 8] rows (xyz, dir, dt, t) of a MarchOut."""
    rows = torch.cat([out.xyzs, out.dirs, out.deltas], -1)
    return [rows[o:o + c].clone() for o, c in out.rays[:, 1:].tolist()]


def _assemble(per_ray, offset_shift=None):
    counts = torch.tensor([r.shape[0] for r in per_ray], dtype=torch.int64)
    offsets = torch.cumsum(counts, 0) - counts
    if offset_shift is not None:
        offsets[offset_shift] += 1
    rows = torch.cat(per_ray, 0)
    rays = torch.stack([torch.arange(len(per_ray)), offsets, counts], -1).to(torch.int32)
    counter = torch.tensor([int(counts.sum()), int((counts > 0).sum()), 0], dtype=torch.int32)
    return R.MarchOut(rays, rows[:, :3].contiguous(), rows[:, 3:6].contiguous(), rows[:, 6:8].contiguous(), counter)


def _lattice_row(case, n, k):
    """The sample row of lattice point k of ray n, as a march would emit it."""
    ref = case.ref
    t = np.float32(ref.t[n, k])
    x = np.clip(ref.o[n] + np.float64(t) * ref.d[n], -case.cfg[0], case.cfg[0]).astype(np.float32)
    return torch.from_numpy(np.concatenate([x, ref.d[n].astype(np.float32), [np.float32(ref.dt[n, k]), t]]).astype(np.float32))


def _insert(case, out, n, k):
    per_ray = _rows(out)
    r = per_ray[n]
    at = int((r[:, 7].double() < case.ref.t[n, k]).sum())
    per_ray[n] = torch.cat([r[:at], _lattice_row(case, n, k)[None], r[at:]], 0)
    return _assemble(per_ray)


def _rejects(name, out, rule):
    with pytest.raises(AssertionError, match=r"march rule \[%s\]" % rule):
        R.assert_case(name, out)


def _interior_ray(case, out, want_cls):
    """(ray, lattice point) of an uncapped ray with >= 8 samples that has a point of class want_cls between its first
    and last sample."""
    ref = case.ref
    for n in range(ref.o.shape[0]):
        c = int(out.rays[n, 2])
        if 8 <= c < case.cfg[3] and ref.hit[n] == 1:
            o = int(out.rays[n, 1])
            lo, hi = float(out.deltas[o, 1]), float(out.deltas[o + c - 1, 1])
            ks = np.nonzero((ref.cls[n] == want_cls) & (ref.t[n] > lo + ref.dt[n]) & (ref.t[n] < hi - ref.dt[n]))[0]
            if len(ks):
                return n, int(ks[len(ks) // 2])
    raise AssertionError("no such ray in " + case.name)


@pytest.mark.parametrize("name", ["plain-random30", "cascade3-random30", "workload-isolated"])
def test_rejects_a_dropped_interior_sample(name):
    case, out = R.build_case(name), R.oracle_march(name)
    n, k = _interior_ray(case, out, R.MUST)
    per_ray = _rows(out)
    i = int((per_ray[n][:, 7].double() - case.ref.t[n, k]).abs().argmin())
    per_ray[n] = torch.cat([per_ray[n][:i], per_ray[n][i + 1:]], 0)
    _rejects(name, _assemble(per_ray), "must")


@pytest.mark.parametrize("name", ["plain-random30", "steplevel-checker", "bound1p5-planes"])
def test_rejects_an_extra_sample_at_an_empty_point(name):
    case, out = R.build_case(name), R.oracle_march(name)
    n, k = _interior_ray(case, out, R.EMPTY)
    _rejects(name, _insert(case, out, n, k), "must-not")


@pytest.mark.parametrize("name", ["plain-full", "cascade3-full", "inverted64-random30"])
def test_rejects_a_lattice_shifted_by_half_a_step(name):
    out = R.oracle_march(name)
    deltas = out.deltas.clone()
    deltas[:, 1] += 0.5 * deltas[:, 0]
    _rejects(name, out._replace(deltas=deltas), "lattice")


def _march_with(monkeypatch, name, cell_index):
    monkeypatch.setattr(O, "march_cell_index", cell_index)
    out = R.oracle_march.__wrapped__(name)
    monkeypatch.undo()
    return out


@pytest.mark.parametrize("name", ["plain-random30", "workload-isolated", "cap100-planes"])
def test_rejects_x_and_z_swapped_in_the_cell_lookup(monkeypatch, name):
    real = O.march_cell_index
    out = _march_with(monkeypatch, name, lambda x, dt, *a: real(x.flip(-1), dt, *a))
    _rejects(name, out, "(must|must-not)")


@pytest.mark.parametrize("name", ["cap100-random30", "cascade3-ring", "steplevel-random30", "bound1p5-checker"])
def test_rejects_a_level_off_by_one(monkeypatch, name):
    real = O.march_cell_index
    bound, cascade, G = R.CONFIGS[name.split("-")[0]][:3]

    def wrong(x, dt, *a):
        # one level up (the last one: one down), the cell taken in that level's box
        idx = real(x, dt, *a)
        level = idx // G ** 3
        other = torch.where(level + 1 < cascade, level + 1, level - 1)
        mip = torch.minimum(torch.pow(torch.tensor(2.0), other.float()), torch.tensor(float(bound)))
        u = ((x / mip[..., None] + 1.0) * (0.5 * G)).clamp(0.0, float(G - 1))
        return other * G ** 3 + O.morton3d(u.to(torch.int64))
    _rejects(name, _march_with(monkeypatch, name, wrong), "(must|must-not)")


@pytest.mark.parametrize("name", ["plain-full", "steplevel-full", "plain-random30-innerbox"])
def test_rejects_a_sample_at_or_past_far(name):
    case, out = R.build_case(name), R.oracle_march(name)
    ref = case.ref
    n = next(n for n in range(ref.o.shape[0]) if ref.hit[n] == 1 and 0 < int(out.rays[n, 2]) < case.cfg[3])
    k = int(np.nonzero(ref.cls[n] == R.PAST_FAR)[0][0])
    _rejects(name, _insert(case, out, n, k), "must-not")


def test_rejects_a_capped_ray_with_more_than_max_steps():
    name = "cap100-full"
    case, out = R.build_case(name), R.oracle_march(name)
    n = int((out.rays[:, 2] == 100).nonzero()[0])
    last_t = float(out.deltas[int(out.rays[n, 1]) + 99, 1])
    k = int(np.nonzero((case.ref.cls[n] == R.MUST) & (case.ref.t[n] > last_t + 0.5 * case.ref.dt[n]))[0][0])
    _rejects(name, _insert(case, out, n, k), "cap")


@pytest.mark.parametrize("name", ["plain-random30", "cap100-full"])
def test_rejects_an_offset_off_by_one(name):
    out = R.oracle_march(name)
    n = int((out.rays[:, 2] > 0).nonzero()[2])
    _rejects(name, _assemble(_rows(out), offset_shift=n), "offsets")


def test_rejects_wrong_totals_and_samples_on_a_miss():
    name = "plain-random30"
    case, out = R.build_case(name), R.oracle_march(name)
    _rejects(name, out._replace(counter=out.counter + torch.tensor([0, 1, 0], dtype=torch.int32)), "counter")
    per_ray = _rows(out)
    per_ray[case.edge["inface"]] = per_ray[0][:1].clone()
    _rejects(name, _assemble(per_ray), "miss")


def test_capacity_rule_through_the_checker():
    """Under capacity M // 3 the checker wants apply_capacity's spans and totals, given the uncapped rays."""
    name = "plain-random30"
    out = R.oracle_march(name)
    M = int(out.rays[:, 2].sum())
    rays, m, live, dropped = O.apply_capacity(out.rays, M // 3)
    assert dropped > 0 and live > 0
    capped = out._replace(rays=rays, counter=torch.tensor([m, live, dropped], dtype=torch.int32))
    R.assert_case(name, capped, capacity=M // 3, raw_rays=out.rays)
    with pytest.raises(AssertionError, match=r"march rule \[offsets\]"):
        R.assert_case(name, out, capacity=M // 3, raw_rays=out.rays)   # the uncapped rays are not the rule's
