"""Filtered search on the GPU: the masked variants of l2_scan (every S, single query), l2_mfma (RT 1 / 4, QT 1 / 2
with a partial query group) and ivf_scan against the unmasked kernels (exact) and the fp64 masked oracle, the
padding guarantee under per-query masks, ties, id maps, buffer canaries, and the document store on the device."""
import functools

import numpy as np
import pytest
import torch

import filter_cases as C
from rag_llm_k8s_amd.index.flat import FlatL2Index, pack_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLT_MAX = C.FLT_MAX
CASES = pytest.mark.parametrize("N,d,nq,k", C.FLAT_CASES)


def _dev_masks(m):
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int32)).to(DEV)


def _dev_q(qmask):
    return torch.from_numpy(np.asarray(qmask, dtype=np.int32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _store(N, d, nq):
    """(xb, q on the host; xt [d][cap], q on the device) of a case, uploaded once."""
    from rag_llm_k8s_amd.ops import native

    xb, q = C.data(N, d, nq)
    cap = N + 17
    xt = torch.zeros(d, cap, device=DEV)
    native.l2_append(xt, cap, 0, xb.to(DEV))
    return xb, q, xt, cap, q.to(DEV)


def _is_mfma(nq, k, d):
    return nq >= 16 and k <= 8 and d % 32 == 0 and d <= 1024


# ------------------------------------------------------------------------------------------ flat kernels
@CASES
def test_all_ones_mask_and_no_filter_equal_unmasked(native, N, d, nq, k):
    xb, q, xt, cap, qd = _store(N, d, nq)
    D0, I0 = native.l2_search(xt, cap, N, qd, k)
    ones = _dev_masks(pack_masks(np.ones((2, N), dtype=bool)))
    for qmask in (np.zeros(nq), np.full(nq, -1), np.arange(nq) % 3 - 1):
        D, I = native.l2_search(xt, cap, N, qd, k, masks=ones, qmask=_dev_q(qmask))
        assert torch.equal(D, D0) and torch.equal(I, I0)


@CASES
def test_knock_out_the_winner_is_exact(native, N, d, nq, k):
    """Each query's own top-1 masked off (one bitmap row per query): the masked top-k is the unmasked
    [1 : k + 1], ids and distances bit for bit. Fails if a kernel ignores the mask, reads another query's row
    or perturbs a distance."""
    xb, q, xt, cap, qd = _store(N, d, nq)
    kk = min(k, 63)
    assert _is_mfma(nq, kk, d) == _is_mfma(nq, kk + 1, d)  # both searches run the same kernel
    D0, I0 = native.l2_search(xt, cap, N, qd, kk + 1)
    al = np.ones((nq, N), dtype=bool)
    al[np.arange(nq), I0[:, 0].cpu().numpy()] = False
    D, I = native.l2_search(xt, cap, N, qd, kk, masks=_dev_masks(pack_masks(al)), qmask=_dev_q(np.arange(nq)))
    assert torch.equal(I, I0[:, 1:]) and torch.equal(D, D0[:, 1:])


@pytest.mark.parametrize("density", C.DENSITIES)
@CASES
def test_random_masks_match_the_fp64_oracle(native, N, d, nq, k, density):
    xb, q, xt, cap, qd = _store(N, d, nq)
    allowed, masks, qmask = C.random_masks(N, nq, density)
    D, I = native.l2_search(xt, cap, N, qd, k, masks=_dev_masks(masks), qmask=_dev_q(qmask))
    C.assert_within_two_swaps(D, I, *C.random_mask_oracle(N, d, nq, k, density))
    C.assert_padding(D, I, allowed.sum(1))
    Ic = I.cpu().numpy()
    assert all(allowed[j, i] for j in range(nq) for i in Ic[j] if i >= 0)


@CASES
def test_bit_boundaries_single_allowed_row(native, N, d, nq, k):
    """Exactly one allowed row at id 0, 31, 32, 63, 64, N - 1: top-1 is that id, the rest is padding."""
    xb, q, xt, cap, qd = _store(N, d, nq)
    ids = np.array([0, 31, 32, 63, 64, N - 1])
    al = np.zeros((6, N), dtype=bool)
    al[np.arange(6), ids] = True
    masks = _dev_masks(pack_masks(al))
    for shift in range(0, 6, nq):  # every boundary is seen by some query
        qmask = (np.arange(nq) + shift) % 6
        D, I = native.l2_search(xt, cap, N, qd, k, masks=masks, qmask=_dev_q(qmask))
        D, I = D.cpu(), I.cpu()
        assert I[:, 0].tolist() == ids[qmask].tolist()
        ref = ((xb[torch.from_numpy(ids[qmask])].double() - q.double()) ** 2).sum(1).float()
        assert torch.allclose(D[:, 0], ref, rtol=1e-4, atol=1e-3)
        C.assert_padding(D, I, [1] * nq)


@CASES
def test_fewer_than_k_and_zero_allowed_pad_exactly(native, N, d, nq, k):
    """Neighbouring queries of one block carry different masks (0, 1, k - 1 and all rows allowed): every
    allowed row comes back, the tail is exactly (-1, FLT_MAX), no id >= 0 is paired with FLT_MAX (the kernels'
    candidate id is per query, not shared by the block)."""
    xb, q, xt, cap, qd = _store(N, d, nq)
    g = np.random.default_rng(11)
    al = np.zeros((4, N), dtype=bool)
    al[1, N // 2] = True
    al[2, g.choice(N, k - 1, replace=False)] = True
    al[3] = True
    for shift in range(0, 4, nq):
        qmask = (np.arange(nq) + shift) % 4
        D, I = native.l2_search(xt, cap, N, qd, k, masks=_dev_masks(pack_masks(al)), qmask=_dev_q(qmask))
        C.assert_padding(D, I, al[qmask].sum(1))
        Ic = I.cpu().numpy()
        for j in range(nq):
            if qmask[j] < 3:
                assert sorted(i for i in Ic[j] if i >= 0) == np.nonzero(al[qmask[j]])[0].tolist()


@CASES
def test_ties_after_masking_the_lowest_duplicate(native, N, d, nq, k):
    """Every vector 4 times (rows i, i + n4, i + 2 n4, i + 3 n4), the lowest-id duplicate of each queried vector
    masked off: the other three come out first, in ascending id order, as exact ties -- at distance exactly 0
    on the direct-form scan. The MFMA path computes ||x||^2 + ||q||^2 - 2 x.q: with q == x these are three
    length-d fp32 fmaf chains over the same sum S = ||x||^2, each within d * 2^-24 * S of it in the worst case
    (the standard bound of recursive summation), so the distance is within 4 * d * 2^-24 * S of 0 -- far below
    the ~2 d of an unrelated row."""
    torch.manual_seed(3)
    n4 = N // 4
    base = torch.randn(n4, d)
    xb = base.repeat(4, 1)
    n = 4 * n4
    xt = torch.zeros(d, n + 5, device=DEV)
    native.l2_append(xt, n + 5, 0, xb.to(DEV))
    al = np.ones((1, n), dtype=bool)
    al[0, :nq] = False
    D, I = native.l2_search(xt, n + 5, n, base[:nq].to(DEV), k, masks=_dev_masks(pack_masks(al)),
                            qmask=_dev_q(np.zeros(nq)))
    D, I = D.cpu(), I.cpu()
    for j in range(nq):
        assert I[j, :3].tolist() == [j + n4, j + 2 * n4, j + 3 * n4]
        assert D[j, 0] == D[j, 1] == D[j, 2]
    if _is_mfma(nq, k, d):
        bound = 4 * d * 2.0 ** -24 * float((base[:nq] ** 2).sum(1).max())
        print("max tie distance %.3g, bound %.3g" % (float(D[:, :3].max()), bound))
        assert 0.0 <= float(D[:, :3].min()) and float(D[:, :3].max()) <= bound
    else:
        assert float(D[:, :3].abs().max()) == 0.0


@CASES
def test_ids_map_row_begin_and_short_bitmap(native, N, d, nq, k):
    """The bitmap is indexed by the MAPPED id (ids_map = 3 row + 11); rows before row_begin are not scanned;
    a mapped id >= mask_bits is not allowed, whatever lies in the words past it."""
    xb, q, xt, cap, qd = _store(N, d, nq)
    ids = torch.arange(cap, dtype=torch.int32) * 3 + 11
    row_begin = N // 5 + 1
    bits = N + 7  # rows with 3 row + 11 >= bits (from about N / 3 on) are cut off
    g = np.random.default_rng(5)
    rows = g.random((2, 32 * ((bits + 31) // 32))) < 0.5  # set bits past mask_bits too
    masks = pack_masks(rows)
    qmask = (np.arange(nq) + 1) % 3 - 1  # 0, 1, -1, ...
    D, I = native.l2_search(xt, cap, N, qd, k, row_begin=row_begin, ids_map=ids.to(DEV), masks=_dev_masks(masks),
                            qmask=_dev_q(qmask), mask_bits=bits)
    mapped = ids[:N].numpy().astype(np.int64)
    allowed = np.ones((nq, N), dtype=bool)
    for j in range(nq):
        if qmask[j] >= 0:
            allowed[j] = (mapped < bits) & rows[qmask[j]][np.minimum(mapped, rows.shape[1] - 1)]
    allowed[:, :row_begin] = False
    Dr, Ir = C.masked_oracle(xb, q, k, allowed, ids=ids.long())
    C.assert_within_two_swaps(D, I, Dr, Ir)
    C.assert_padding(D, I, allowed.sum(1))
    with pytest.raises(ValueError):
        native.l2_search(xt, cap, N, qd, k, masks=_dev_masks(masks), qmask=_dev_q(qmask),
                         mask_bits=32 * masks.shape[1] + 1)  # a bitmap row shorter than mask_bits
    with pytest.raises(ValueError):
        native.l2_search(xt, cap, N, qd, k, masks=_dev_masks(masks), qmask=_dev_q(np.full(nq, 2)))  # no such row


@pytest.mark.parametrize("nq,k", [(5, 4), (20, 4)])  # scan and MFMA
def test_masked_search_guard_canaries(native, nq, k):
    """Partial lists, outputs, bitmaps and qmask in sentinel-padded allocations sized exactly (the buffers of
    test_l2_search_guard_canaries): nothing outside the views changes, and the entry point refuses a bitmap row
    shorter than mask_bits."""
    torch.manual_seed(4)
    N, d = 7777, 384
    cap = N + 3
    xt = torch.zeros(d, cap, device=DEV)
    native.l2_append(xt, cap, 0, torch.randn(N, d, device=DEV))
    L = native._lib.lib()
    G = L.ragk_l2_search_groups(0, N, nq, k, d)
    pad = 4096
    q = torch.randn(nq, d, device=DEV)
    sizes = (nq * G * k, nq * k)
    bufs = [torch.full((2 * pad + n,), -7.0, device=DEV) for n in sizes]
    ibufs = [torch.full((2 * pad + n,), -7, dtype=dt, device=DEV) for n, dt in zip(sizes, (torch.int32, torch.int64))]
    views = [b[pad:pad + n] for b, n in zip(bufs, sizes)]
    iviews = [b[pad:pad + n] for b, n in zip(ibufs, sizes)]
    allowed, masks, qmask = C.random_masks(N, nq, 0.5)
    words = masks.shape[1]
    mbuf = torch.full((2 * pad + nq * words,), -7, dtype=torch.int32, device=DEV)
    mview = mbuf[pad:pad + nq * words]
    mview.copy_(_dev_masks(masks).reshape(-1))
    qbuf = torch.full((2 * pad + nq,), -7, dtype=torch.int32, device=DEV)
    qview = qbuf[pad:pad + nq]
    qview.copy_(_dev_q(qmask))
    before = mview.clone()

    def call(bits):
        return L.ragk_l2_search_masked(xt.data_ptr(), cap, d, 0, N, q.data_ptr(), nq, k, None, mview.data_ptr(), words,
                                       bits, qview.data_ptr(), views[0].data_ptr(), iviews[0].data_ptr(),
                                       views[1].data_ptr(), iviews[1].data_ptr(), native.stream_ptr())

    assert call(32 * words + 1) != 0  # hipErrorInvalidValue before any launch
    native.check(call(N), "ragk_l2_search_masked")
    torch.cuda.synchronize()
    for b, ib in zip(bufs, ibufs):
        assert b[:pad].eq(-7.0).all() and b[-pad:].eq(-7.0).all()
        assert ib[:pad].eq(-7).all() and ib[-pad:].eq(-7).all()
    for b in (mbuf, qbuf):
        assert b[:pad].eq(-7).all() and b[-pad:].eq(-7).all()
    assert torch.equal(mview, before)
    Dr, Ir = C.masked_oracle(xt[:, :N].t().cpu(), q.cpu(), k, allowed)
    C.assert_within_two_swaps(views[1].view(nq, k), iviews[1].view(nq, k), Dr, Ir)


# ------------------------------------------------------------------------------------------ IVF
@functools.lru_cache(maxsize=None)
def _ivf():
    from rag_llm_k8s_amd.index.ivf import IVFFlatIndex

    N, d, nlist = C.IVF_CASE
    xb, q = C.data(N, d, 9)
    idx = IVFFlatIndex(d, device=DEV, nlist=nlist, nprobe=nlist)
    idx.train(xb)
    idx.add(xb)
    return idx, xb, q


def _ivf_host(idx, q, k, masks=None, qmask=None):
    """The CPU search of the same index with the probes the device search uses."""
    pr = idx._coarse_device(q.to(DEV), min(idx.nprobe, idx.nlist)).cpu()
    return idx._search_host(q, pr, k, masks, qmask)


@pytest.mark.parametrize("nprobe", [16, 4])
def test_ivf_masked_search(native, nprobe):
    idx, xb, q = _ivf()
    idx.nprobe = nprobe
    N, nq, k = xb.shape[0], q.shape[0], 6
    D0, I0 = idx.search(q, k + 1)
    # all ones / no filter == unmasked, bit for bit
    ones = pack_masks(np.ones((1, N), dtype=bool))
    for qmask in (np.zeros(nq), np.full(nq, -1)):
        D, I = idx.search(q, k + 1, masks=ones, qmask=qmask)
        assert torch.equal(D, D0) and torch.equal(I, I0)
    # knock out each query's winner: exactly the unmasked [1 : k + 1]
    al = np.ones((nq, N), dtype=bool)
    al[np.arange(nq), I0[:, 0].numpy()] = False
    D, I = idx.search(q, k, masks=pack_masks(al), qmask=np.arange(nq))
    assert torch.equal(I, I0[:, 1:]) and torch.equal(D, D0[:, 1:])
    # random masks mixed with -1 against the CPU search with the same probes
    for density in C.DENSITIES:
        allowed, masks, qmask = C.random_masks(N, nq, density)
        D, I = idx.search(q, k, masks=masks, qmask=qmask)
        Dh, Ih = _ivf_host(idx, q, k, masks, qmask)
        C.assert_within_two_swaps(D, I, Dh, Ih)
        assert all(allowed[j, i] for j in range(nq) for i in I[j].tolist() if i >= 0)
        assert not bool(((I >= 0) & (D == FLT_MAX)).any())
    # bit boundaries and fewer than k / zero allowed, a different mask on every query
    ids = np.array([0, 31, 32, 63, 64, N - 1])
    al = np.zeros((9, N), dtype=bool)
    al[np.arange(6), ids] = True
    al[7, np.random.default_rng(2).choice(N, k - 1, replace=False)] = True
    al[8] = True
    masks, qmask = pack_masks(al), np.arange(nq)
    D, I = idx.search(q, k, masks=masks, qmask=qmask)
    Dh, Ih = _ivf_host(idx, q, k, masks, qmask)
    assert torch.equal(I, Ih) and torch.allclose(D, Dh, rtol=1e-4, atol=1e-3)
    assert not bool(((I >= 0) & (D == FLT_MAX)).any()) and bool((I[6] == -1).all()) and bool((D[6] == FLT_MAX).all())
    if nprobe == 16:  # every list probed: each single allowed row is found
        assert I[:6, 0].tolist() == ids.tolist() and bool((I[:6, 1:] == -1).all()) and bool((I[7, :k - 1] >= 0).all())
        C.assert_padding(D, I, al.sum(1))


def test_ivf_ties_after_masking_the_lowest_duplicate(native):
    from rag_llm_k8s_amd.index.ivf import IVFFlatIndex

    torch.manual_seed(3)
    base = torch.randn(750, 64)
    idx = IVFFlatIndex(64, device=DEV, nlist=16, nprobe=16)
    idx.train(base)
    idx.add(base.repeat(4, 1))
    al = np.ones((1, 3000), dtype=bool)
    al[0, :7] = False
    D, I = idx.search(base[:7], 5, masks=pack_masks(al), qmask=np.zeros(7))
    for j in range(7):
        assert I[j, :3].tolist() == [j + 750, j + 1500, j + 2250]
    assert float(D[:, :3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ stores on the device
@pytest.mark.parametrize("index_type", ["flat", "ivf"])
def test_store_delete_filter_compact_gpu(native, tmp_path, index_type):
    C.store_scenario(tmp_path, "cuda", index_type)


def _flat_dev(xb):
    idx = FlatL2Index(xb.shape[1], device=DEV)
    idx.add(xb)
    return idx


def test_flat_compact_on_the_device_equals_fresh_index(native):
    xb, q = C.data(5000, 96, 7, seed=4)
    keep = np.sort(np.random.default_rng(0).choice(5000, 2111, replace=False))
    idx = _flat_dev(xb)
    idx.compact(keep)
    fresh = _flat_dev(xb[torch.from_numpy(keep)])
    assert idx.ntotal == fresh.ntotal == 2111
    for kk, qq in ((9, q), (4, q.repeat(3, 1))):  # scan and MFMA
        D, I = idx.search(qq, kk)
        Df, If = fresh.search(qq, kk)
        assert torch.equal(D, Df) and torch.equal(I, If)
    assert np.array_equal(idx.reconstruct_all(), xb[torch.from_numpy(keep)].numpy())
    idx.add(xb[:3])
    assert idx.ntotal == 2114 and np.array_equal(idx.reconstruct_all()[2111:], xb[:3].numpy())
    # masked search of the compacted index: ids are the new ranks
    allowed, masks, qmask = C.random_masks(2114, 7, 0.5)
    D, I = idx.search(q, 9, masks=masks, qmask=qmask)
    cur = torch.cat([xb[torch.from_numpy(keep)], xb[:3]])
    C.assert_within_two_swaps(D, I, *C.masked_oracle(cur, q, 9, allowed))


def test_flat_compact_50k_every_other_row(native):
    """50k x 384 with every other row dropped: compacted in place in bounded pieces (more than one piece at
    this size), equal to a fresh index of the kept rows."""
    torch.manual_seed(8)
    xb = torch.randn(50000, 384)
    idx = _flat_dev(xb)
    from rag_llm_k8s_amd.index.flat import COMPACT_PIECE_FLOATS

    assert COMPACT_PIECE_FLOATS // 384 < 25000 // 2  # the kept rows span more than two gather / append pieces
    cap = idx._cap
    idx.compact(np.arange(0, 50000, 2))
    assert idx.ntotal == 25000 and idx._cap == cap  # no second store
    assert np.array_equal(idx.reconstruct_all(), xb[::2].numpy())
    q = xb[[1, 2, 49999]] + 0.01
    D, I = idx.search(q, 4)
    Df, If = _flat_dev(xb[::2].contiguous()).search(q, 4)
    assert torch.equal(D, Df) and torch.equal(I, If)
    assert I[1, 0].item() == 1  # old row 2 is new id 1
