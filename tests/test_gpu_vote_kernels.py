"""The majority-vote kernels on the MI355X against their numpy restatement (include/fedvote.h): ``count_votes`` is the
integer column sum of the unpacked bits, exactly, either side of every adder group, dword, strip and tile, on every
launch level and with the rows split or not; ``finish_vote`` is three fp32 numpy operations, bit for bit; ``vote_row``
gives the host encoder's bytes.

The kernel takes its number of high planes (H = 4, 8, 12) from the rows ONE workgroup counts — n, or a slice of a
split plan — so the plane edges 256 and 4096 are edges of that number, not of n.  The issue's n (255 .. 4097, 65535)
stay as cases; at their P they are split into slices below 4096 rows, so ``BIG`` adds shapes chosen from the plan at
the device's CU count whose workgroups count 4095, 4096 and 4097 rows unsplit, 4080 and 4096 rows as slices, and 1000
and 4096 rows on the capped grid, and ``test_every_kernel_variant_is_launched`` asserts from the plan that every
(plain / atomic / capped grid) x H kernel the library can launch is launched by some case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_N, EDGE_N = (1, 15, 16, 17, 33), (255, 256, 257, 4095, 4096, 4097)
EDGE_P = (1, 31, 33, 2047, 2049, 8191, 8193)
CASES = sorted({(n, P) for n in SMALL_N for P in (33, 8193)} | {(n, P) for n in EDGE_N for P in (31, 2049)}
               | {(n, P) for P in EDGE_P for n in (17, 257)} | {(65535, 2049)})


def _rows(n, P, seed=11):
    """(packed [n, ldb] uint8, counts int64 [P]): Bernoulli(q_p) bits, q_p = 0 / 1 at p % 5 == 0 / 1."""
    from fedscale_amd.kernels_vote import bit_stride

    rng = np.random.default_rng(seed)
    q = rng.random(P, dtype=np.float32)
    q[0::5], q[1::5] = 0.0, 1.0
    packed = np.zeros((n, bit_stride(P)), dtype=np.uint8)
    for k in range(0, n, 8192):
        b = rng.random((min(8192, n - k), P), dtype=np.float32) < q
        packed[k:k + b.shape[0], :(P + 7) // 8] = np.packbits(b, axis=1, bitorder="little")
    want = np.zeros(P, dtype=np.int64)
    for k in range(0, n, 8192):
        want += np.unpackbits(packed[k:k + 8192], axis=1, bitorder="little")[:, :P].sum(axis=0, dtype=np.int64)
    return packed, want


def _count(dev, packed, n, P, cnt=None, **kw):
    from fedscale_amd.kernels_vote import count_votes

    if cnt is None:
        cnt = torch.full((P + 68,), -7, dtype=torch.int32, device=dev)
    count_votes(torch.from_numpy(packed).to(dev), n, P, cnt, **kw)
    got = cnt.cpu().numpy()
    assert (got[P:] == -7).all(), "columns at and beyond P are untouched"
    return cnt, got[:P].astype(np.int64)


def _plan_P(cus):
    """Two more P from the plan: one whose plan has a whole-tile and a ragged launch, one with a capped grid."""
    from fedscale_amd.kernels_vote import count_votes_plan

    P12, P0 = (4 * ((cus + 1) // 2) + 1) * 2048 - 5, (8 * cus + 3) * 8192 + 77
    assert len(count_votes_plan(cus, 17, P12)) == 2
    (l0,) = count_votes_plan(cus, 17, P0)
    assert l0["grid"] < l0["tiles"]
    return P12, P0


def _rows_dev(dev, n, P, seed=5):
    """(bits [n, ldb] on the device, counts int64 [P]) for shapes too large to draw on the host: uniform random bytes
    (q_p = 1/2) with the columns p % 5 == 0 / 1 forced to 0 / 1 and the padding bits to 0 by byte masks, so counts of
    0 and of n occur; tallied by torch integer ops, 64 rows at a time."""
    from fedscale_amd.kernels_vote import bit_stride

    ldb = bit_stride(P)
    col = np.arange(8 * ldb)
    keep = torch.from_numpy(np.packbits((col % 5 != 0) & (col < P), bitorder="little")).to(dev)
    force = torch.from_numpy(np.packbits((col % 5 == 1) & (col < P), bitorder="little")).to(dev)
    bits = torch.empty(n, ldb, dtype=torch.uint8, device=dev)
    bits.random_(0, 256, generator=torch.Generator(device=dev).manual_seed(seed))
    bits.bitwise_and_(keep).bitwise_or_(force)
    acc = torch.zeros(ldb, 8, dtype=torch.int64, device=dev)
    for k in range(0, n, 64):
        for i in range(8):
            acc[:, i] += ((bits[k:k + 64] >> i) & 1).sum(0, dtype=torch.int64)
    return bits, acc.reshape(-1)[:P].cpu().numpy()


def _variants(cus, n, P):
    """({(kind, H)} of the kernels fvt_count launches at (n, P), launches, S), from the plan export."""
    from fedscale_amd.kernels_vote import count_votes_plan

    plan = count_votes_plan(cus, n, P)
    S = plan[0]["S"]
    rows = n if S == 1 else -(-(-(-n // S)) // 16) * 16  # of one workgroup: round_up(ceil(n / S), 16) when split
    H = 4 if rows < 256 else 8 if rows < 4096 else 12
    return {("loop" if l["grid"] < l["tiles"] else "atomic" if S > 1 else "plain", H) for l in plan}, len(plan), S


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# name -> (n, P(cus), the kernels it must launch, S).  full: as many tiles as CUs, never split; two: just over two
# thirds of the CUs in tiles, split in two; P12 / P0: _plan_P's two-launch and capped-grid shapes.
BIG = {
    "plain-4095": (4095, lambda c: (c - 1) * 8192 + 1, {("plain", 8)}, 1),
    "plain-4096": (4096, lambda c: (c - 1) * 8192 + 1, {("plain", 12)}, 1),
    "plain-4097": (4097, lambda c: (c - 1) * 8192 + 1, {("plain", 12)}, 1),
    "atomic-8160": (8160, lambda c: (2 * c // 3) * 8192 + 1, {("atomic", 8)}, 2),
    "atomic-8161": (8161, lambda c: (2 * c // 3) * 8192 + 1, {("atomic", 12)}, 2),
    "atomic-8192": (8192, lambda c: (2 * c // 3) * 8192 + 1, {("atomic", 12)}, 2),
    "two-launches-split-1000": (1000, lambda c: _plan_P(c)[0], {("atomic", 8)}, 3),
    "loop-1000": (1000, lambda c: _plan_P(c)[1], {("loop", 8)}, 1),
    "loop-4096": (4096, lambda c: _plan_P(c)[1], {("loop", 12)}, 1),
}


@pytest.mark.parametrize("name", list(BIG))
def test_count_votes_at_the_plane_edges_of_every_kernel(gpu_device, name):
    from fedscale_amd.kernels_vote import count_votes

    n, P_of, kernels, S = BIG[name]
    cus = _cus(gpu_device)
    P = P_of(cus)
    got_k, launches, got_S = _variants(cus, n, P)
    assert got_k == kernels and got_S == S
    assert launches == (1 if name.startswith("loop") else 2)
    bits, want = _rows_dev(gpu_device, n, P)
    cnt = torch.full((P + 68,), -7, dtype=torch.int32, device=gpu_device)
    count_votes(bits, n, P, cnt)
    got = cnt.cpu().numpy()
    assert np.array_equal(got[:P].astype(np.int64), want) and (got[P:] == -7).all()
    assert want[0] == 0 and want[1] == n and 0 < want[2] < n


def test_every_kernel_variant_is_launched(gpu_device):
    cus = _cus(gpu_device)
    seen = set()
    for n, P in CASES + [(2, _plan_P(cus)[0]), (17, _plan_P(cus)[1])] + [(v[0], v[1](cus)) for v in BIG.values()]:
        seen |= _variants(cus, n, P)[0]
    # a split slice is at least 256 rows: ("atomic", 4) does not exist in the library
    assert seen == {(k, H) for k in ("plain", "atomic", "loop") for H in (4, 8, 12)} - {("atomic", 4)}


@pytest.mark.parametrize("n,P", CASES)
def test_count_votes_is_the_integer_sum(gpu_device, n, P):
    packed, want = _rows(n, P)
    assert np.array_equal(_count(gpu_device, packed, n, P)[1], want)
    if n == 33:
        assert want.min() == 0 and want.max() == n


def test_the_cases_split_rows_and_do_not(gpu_device):
    from fedscale_amd.kernels_vote import count_votes_plan

    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    S = {c: count_votes_plan(cus, *c)[0]["S"] for c in CASES}
    assert S[(4097, 2049)] > 1 and S[(33, 8193)] == 1 and min(S.values()) == 1


@pytest.mark.parametrize("which,n", [(0, 2), (0, 257), (1, 2), (1, 17)])
def test_count_votes_on_every_launch_level(gpu_device, which, n):
    P = _plan_P(torch.cuda.get_device_properties(gpu_device).multi_processor_count)[which]
    packed, want = _rows(n, P)
    assert np.array_equal(_count(gpu_device, packed, n, P)[1], want)


@pytest.mark.parametrize("n1,n2,P", [(17, 16, 2049), (17, 16, 8193), (1025, 1024, 2049)])
def test_accumulate_is_one_call(gpu_device, n1, n2, P):
    """(17, 16): the issue's rows, which no plan splits; (1025, 1024) splits both calls on any MI355X."""
    packed, want = _rows(n1 + n2, P)
    cnt, got1 = _count(gpu_device, packed[:n1], n1, P)
    _, got = _count(gpu_device, packed[n1:], n2, P, cnt=cnt, accumulate=True)
    assert np.array_equal(got, want) and np.array_equal(_count(gpu_device, packed, n1 + n2, P)[1], want)


def _finish_want(c, L, K, eta, mode):
    v = K - 2 * c.astype(np.int64)
    eta = np.float32(eta)
    if mode == "majority":
        s = np.where(v > 0, eta, np.where(v < 0, -eta, np.float32(0.0))).astype(np.float32)
    else:
        s = eta * (v.astype(np.float32) / np.float32(K))
    return L + s


@pytest.mark.parametrize("mode", ["majority", "mean"])
@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("eta", [1e-3, float(np.float32(1 / 3))])
@pytest.mark.parametrize("P", [1, 5, 1027])
def test_finish_vote_bit_for_bit(gpu_device, mode, K, eta, P):
    from fedscale_amd.kernels_vote import finish_vote

    rng = np.random.default_rng(P)
    c = np.resize(np.array([0, K, K // 2, K // 2 + 1, max(K // 2 - 1, 0)], dtype=np.int32), P)
    L = rng.standard_normal(P).astype(np.float32)
    special = np.array([-0.0, 1e-40, 1e30, 0.0], dtype=np.float32)
    L[:min(P, 4)] = special[:min(P, 4)]
    L[5::6] = np.resize(special, L[5::6].size)
    out = torch.full((P + 4,), 9.0, dtype=torch.float32, device=gpu_device)
    mirror = torch.zeros(P + 4, dtype=torch.float32, device=gpu_device)
    finish_vote(torch.from_numpy(c).to(gpu_device), torch.from_numpy(L).to(gpu_device), P, K, eta, out, mode=mode,
                mirror=mirror)
    want = _finish_want(c, L, K, eta, mode)
    assert np.array_equal(out.cpu().numpy()[:P].view(np.uint32), want.view(np.uint32))
    assert torch.equal(out[:P], mirror[:P]) and (out[P:] == 9.0).all()


@pytest.mark.parametrize("P", [1, 63, 65, 257, 1021])
def test_vote_row_gives_the_host_bytes(gpu_device, P):
    from fedscale_amd.cloud.execution.vote_upload import VOTE_BITS_KEY, compress_vote
    from fedscale_amd.kernels_vote import bit_bytes, vote_row

    rng = np.random.default_rng(P)
    base = rng.standard_normal(P).astype(np.float32)
    x = (base + rng.standard_normal(P).astype(np.float32)).astype(np.float32)
    sp = np.array([0x80000000, 0, 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000], dtype=np.uint32).view(np.float32)
    idx = rng.permutation(P)[:6]
    x[idx] = sp[:idx.size]
    base[idx[:2]] = 0.0  # so that x - base is -0.0 and +0.0 there
    want = compress_vote({"w": x}, {"w": base})[VOTE_BITS_KEY]
    bits = torch.full((bit_bytes(P) + 8,), 0xAA, dtype=torch.uint8, device=gpu_device)
    vote_row(torch.from_numpy(x).to(gpu_device), torch.from_numpy(base).to(gpu_device), P, bits)
    got = bits.cpu().numpy()
    assert np.array_equal(got[:bit_bytes(P)], want) and (got[bit_bytes(P):] == 0xAA).all()
    assert P % 8 == 0 or got[bit_bytes(P) - 1] >> (P % 8) == 0, "the padding bits are 0"
    on_gpu = compress_vote({"w": torch.from_numpy(x).to(gpu_device)}, {"w": torch.from_numpy(base)})[VOTE_BITS_KEY]
    assert np.array_equal(on_gpu, want)
