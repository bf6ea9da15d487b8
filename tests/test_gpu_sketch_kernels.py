"""On the MI355X: the Count-Sketch kernels (include/fedsketch.h) against the numpy restatement of
tests/sketch_fixtures.py, bit for bit — fcs_sketch_row at every tile, either side of the loads-in-flight depth and of a
block's end, fcs_estimate on hand-made tables, fcs_state_step and fcs_apply."""
import itertools

import numpy as np
import pytest
import torch

from fedscale_amd import kernels_sketch as kk
from tests import sketch_fixtures as fx

pytestmark = pytest.mark.gpu
T, U = kk.TILE, kk.U
SEEDS = (0, 2 ** 63 + 11)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cases():
    n = 0
    for R, C in ((1, 1024), (3, 2 * T), (5, 4 * T), (7, 1024)):  # the mask's bits above the tile select other tiles
        for P in (1, C - 1, C, C + 1, 3 * C + 5):
            yield R, C, P, SEEDS[n % 2], (0, 1024, 512, 256)[n % 4]
            n += 1
    yield 7, 4 * T, 3 * 4 * T + 5, SEEDS[1], 1024  # seven rows whose masks select other tiles
    for C, NB in itertools.product((1024, 4 * T), (U - 1, U, U + 1, 2 * U + 1)):  # either side of a load group
        yield 5, C, NB * C - (3 if NB % 2 else 0), SEEDS[NB % 2], (1024, 0)[NB % 2]


@pytest.mark.parametrize("R,C,P,seed,tile", list(_cases()))
def test_sketch_row_is_the_restatement(gpu_device, R, C, P, seed, tile):
    rng = np.random.default_rng(P + R)
    x, base = rng.standard_normal(P).astype(np.float32), rng.standard_normal(P).astype(np.float32)
    table = torch.full((R * C,), 7.0, dtype=torch.float32, device=gpu_device)  # every bucket is written
    kk.sketch_row(_dev(x, gpu_device), _dev(base, gpu_device), None, P, R, C, seed, table, tile=tile)
    assert np.array_equal(_bits(table.cpu().numpy()), _bits(fx.sketch(x - base, R, C, seed)).reshape(-1))


@pytest.mark.parametrize("how", ["plain", "residual", "subtract", "special"])
def test_sketch_row_operands_epilogue_and_special_values(gpu_device, how):
    R, C, P, seed = 5, 2 * T, 9 * 2 * T + 77, 5
    rng = np.random.default_rng(4)
    x, r = rng.standard_normal(P).astype(np.float32), rng.standard_normal(P).astype(np.float32)
    t0 = rng.standard_normal(R * C).astype(np.float32)
    table = _dev(t0, gpu_device)
    if how == "special":  # +-0, a subnormal, an infinity and a NaN: the restatement decides what they become
        x[[3, 2 * T + 3, 5000, P - 1, 9000, 12000]] = [0.0, -0.0, 1e-40, -1e-41, np.inf, np.nan]
        x[C:C + 64] = -0.0
        x[:64] = 0.0
    with np.errstate(all="ignore"):
        e = x + r if how == "residual" else x
        want = fx.sketch(e, R, C, seed).reshape(-1)
        want = t0 - want if how == "subtract" else want
    kk.sketch_row(_dev(x, gpu_device), None, _dev(r, gpu_device) if how == "residual" else None, P, R, C, seed, table,
                  subtract=how == "subtract")
    got = table.cpu().numpy()
    nan = np.isnan(want)
    assert how != "special" or (nan.sum() >= R and np.isinf(want).sum() >= 1)
    assert np.array_equal(np.isnan(got), nan)  # (a NaN's payload is the adder's business)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _median(tup):
    return fx.unkeys(np.sort(fx.keys(np.array(tup, dtype=np.float32)))[len(tup) // 2:len(tup) // 2 + 1])[0]


@pytest.mark.parametrize("R,rem", [(1, 0), (3, 1), (5, 2), (7, 3)])
def test_estimate_on_hand_made_tables(gpu_device, R, rem):
    """One column per R-tuple, written into its R buckets by hand: every order of distinct values (a sample of 200 at
    R = 7), ties, -0 against +0, the infinities and both NaNs; the last float4 ragged."""
    C, seed = 1024, 3
    rng = np.random.default_rng(R)
    vals = (np.arange(R) - R // 2 + 0.5).astype(np.float32)
    perms = list(itertools.permutations(vals))
    if R == 7:
        perms = [perms[i] for i in rng.choice(len(perms), 200, replace=False)]
    nan = np.array([0x7FC00001, 0xFFC00001], dtype=np.uint32).view(np.float32)
    pool = [0.0, -0.0, 1.0, 1.0, -1.0, np.inf, -np.inf, nan[0], nan[1], 1e-40, -1e-40]
    tups = perms + [tuple(pool[i] for i in rng.integers(0, len(pool), R)) for _ in range(300)]
    while len(tups) % 4 != rem:
        tups.append(tuple(rng.standard_normal(R)))
    P = len(tups)
    assert P <= C  # one block: a bucket holds one column
    v = np.array(tups, dtype=np.float32).T.copy()  # [R, P]
    table = rng.standard_normal((R, C)).astype(np.float32)
    for j in range(R):
        table[j, fx.buckets(seed, j, P, C)] = (_bits(v[j]) ^ fx.signs(seed, j, P)).view(np.float32)
    est = torch.full((P + 8,), 7.0, dtype=torch.float32, device=gpu_device)
    kk.estimate(_dev(table.reshape(-1), gpu_device), P, R, C, seed, est)
    got = est.cpu().numpy()
    assert np.array_equal(_bits(got[:P]), _bits(np.array([_median(v[:, p]) for p in range(P)], dtype=np.float32)))
    assert (got[P:] == 7.0).all()  # nothing is written past P


@pytest.mark.parametrize("R,C,P", [(5, 2 * T, 3 * 2 * T + 5), (3, 1024, 1024 * 5 + 2)])
def test_estimate_over_several_blocks_is_the_restatement(gpu_device, R, C, P):
    table = np.random.default_rng(P).standard_normal((R, C)).astype(np.float32)
    est = torch.empty(P, dtype=torch.float32, device=gpu_device)
    kk.estimate(_dev(table.reshape(-1), gpu_device), P, R, C, SEEDS[1], est)
    assert np.array_equal(_bits(est.cpu().numpy()), _bits(fx.estimate(table, P, SEEDS[1])))


def test_state_step_and_its_nonfinite_count(gpu_device):
    n, rho = 3 * 1024, 0.9
    rng = np.random.default_rng(0)
    s, su, se = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    s[[5, 1000, 3071]] = [np.inf, -np.inf, np.nan]
    d = [_dev(a, gpu_device) for a in (s, su, se)]
    out_u, out_e = torch.empty_like(d[1]), torch.empty_like(d[2])
    bad = torch.full((1,), 2, dtype=torch.int32, device=gpu_device)
    kk.state_step(d[0], d[1], d[2], rho, n, out_u, out_e, bad)
    with np.errstate(all="ignore"):
        want_u = np.float32(rho) * su + s
        want_e = se + want_u
    ok = np.isfinite(s)
    assert int(bad.item()) == 2 + 3
    assert np.array_equal(_bits(out_u.cpu().numpy())[ok], _bits(want_u)[ok])
    assert np.array_equal(_bits(out_e.cpu().numpy())[ok], _bits(want_e)[ok])
    assert np.array_equal(np.isnan(out_e.cpu().numpy()), np.isnan(want_e))
    kk.state_step(d[0], d[1], d[2], rho, n, d[1], d[2], bad)  # in place
    okd = _dev(ok, gpu_device)
    assert torch.equal(d[1][okd], out_u[okd])


@pytest.mark.parametrize("in_place", [False, True])
def test_apply_densifies_and_moves_only_the_named_columns(gpu_device, in_place):
    P, k = 4099, 37
    rng = np.random.default_rng(2)
    L = rng.standard_normal(P).astype(np.float32)
    L[7] = -0.0
    idx = np.sort(rng.choice(P, k, replace=False)).astype(np.int32)
    idx[-1] = P - 1
    val = rng.standard_normal(k).astype(np.float32)
    l_in = _dev(L, gpu_device)
    l_out = l_in if in_place else torch.full((P,), 7.0, dtype=torch.float32, device=gpu_device)
    dense = torch.full((P,), 7.0, dtype=torch.float32, device=gpu_device)
    kk.apply_pairs(_dev(idx, gpu_device), _dev(val, gpu_device), k, P, dense, l_in, l_out)
    want_d, want_l = np.zeros(P, dtype=np.float32), L.copy()
    want_d[idx] = val
    want_l[idx] = L[idx] + val
    assert np.array_equal(_bits(dense.cpu().numpy()), _bits(want_d))
    assert np.array_equal(_bits(l_out.cpu().numpy()), _bits(want_l))
