"""Every sampled token pinned: the three candidate top-k kernels and sample_candidates_kernel of
csrc/kernels/sampling.hip against the float64 replica of the draw in sampling_cases.py -- the token of every row
(or, on the few rows where fp32 cannot decide a comparison, one of the replica's alternatives), its logprob within
the row's band, the top-k lists element by element with ties to the lowest id. All outputs are written inside
sentinel frames that must stay intact."""
import functools

import numpy as np
import pytest
import torch

import sampling_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 256
GAP = 3.0e30  # fills the gap between the width and the stride of strided logits: read as a logit, it wins
AMBIGUOUS_CAP = 0.02


def _framed(shape, dtype, fill, sentinel):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(*shape)
    view.fill_(fill)
    return buf, view


def _pads_intact(buf, sentinel):
    return bool((buf[:PAD] == sentinel).all()) and bool((buf[-PAD:] == sentinel).all())


def run_sampler(native, cv, ci, p, list_len):
    """One launch over the rows of a table: (tok int64 [B], lp float64 [B]) on the CPU. out_tok / out_lp arrive
    holding a sentinel token / NaN inside sentinel frames: the frames stay, every output is written."""
    B = cv.shape[0]
    tbuf, tok = _framed((B,), torch.int32, S.SENT_TOK, -777)
    lbuf, lp = _framed((B,), torch.float32, float("nan"), -7.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    native.sample_candidates(dev(cv), dev(ci), dev(p["T"]), dev(p["top_k"]), dev(p["top_p"]), dev(p["seed"]),
                             dev(p["step"]), out_tok=tok, out_lp=lp, list_len=list_len)
    torch.cuda.synchronize()
    assert _pads_intact(tbuf, -777) and _pads_intact(lbuf, -7.0)
    tok, lp = tok.cpu().numpy().astype(np.int64), lp.cpu().numpy().astype(np.float64)
    assert (tok != S.SENT_TOK).all() and not np.isnan(lp).any()
    return tok, lp


def check_rows(tok, lp, ref, what):
    """Tokens equal the reference's on unambiguous rows and lie in the alternatives otherwise; logprobs within the
    row's band (greedy and empty rows, band 0: exactly 0 and -inf). Returns (ambiguous share, worst lp error in
    units of the band)."""
    rtok, rlp, band, alts = ref
    amb = np.array([bool(a) for a in alts])
    for b in np.nonzero(amb)[0]:
        assert int(tok[b]) in alts[b], (what, int(b), int(tok[b]), alts[b])
    bad = np.nonzero(~amb & (tok != rtok))[0]
    assert bad.size == 0, (what, "rows", bad[:8].tolist(), "got", tok[bad[:8]].tolist(), "want", rtok[bad[:8]].tolist())
    sure = ~amb & (band > 0)
    err = np.abs(lp[sure] - rlp[sure])
    worst = float((err / band[sure]).max()) if sure.any() else 0.0
    print("%s: ambiguous %.2f%%, worst |lp - ref| / band %.3f" % (what, 100 * amb.mean(), worst))
    assert (err <= band[sure]).all(), (what, worst)
    fixed = ~amb & (band == 0)
    assert np.array_equal(lp[fixed], rlp[fixed]), (what, lp[fixed], rlp[fixed])
    return float(amb.mean()), worst


def _params(t):
    return {k: t[k] for k in ("T", "top_k", "top_p", "seed", "step")}


@functools.lru_cache(maxsize=None)
def _routes():
    t = S.routes_table()
    cv, ci, _ = t["shapes"]["sort"]
    return t, S.ref_rows(cv, ci, t["T"], t["top_k"], t["top_p"], t["seed"], t["step"])


# ----------------------------------------------------------------------------- the sampler
def test_routes(native):
    """Heterogeneous rows through every branch of sample_candidates_kernel: bitonic sort, rank merge, lane-network
    merge, and (rows with K > 64, whatever the shaping) the serial tail."""
    t, ref = _routes()
    k = t["top_k"]
    tail = (k <= 0) | (k > 64)
    assert tail.sum() >= 100 and (~tail).sum() >= 100
    toks = {}
    for name, (cv, ci, L) in t["shapes"].items():
        tok, lp = run_sampler(native, cv, ci, _params(t), L)
        share, _ = check_rows(tok, lp, ref, "routes/" + name)
        assert share <= AMBIGUOUS_CAP
        toks[name] = tok
    sure = np.array([not a for a in ref[3]])
    for name in toks:  # the routes agree row by row
        assert np.array_equal(toks[name][sure], toks["sort"][sure]), name


def test_exact_rows_pin_the_top_p_comparison(native):
    """Four candidates of probability exactly 1/4 and top_p = 1/4, 1/2, 3/4: the mass above candidate i equals
    top_p exactly for one i, and "< top_p" drops that candidate."""
    t = S.exact_table()
    ref = S.ref_rows(t["cv"], t["ci"], t["T"], t["top_k"], t["top_p"], t["seed"], t["step"], exact=True)
    assert len(set(ref[0].tolist())) == 3  # (the fourth candidate is never kept)
    for L in t["list_lens"]:
        cv, ci = zip(*(S.shape_lists(v, i, L or 8) for v, i in zip(t["cv"], t["ci"])))
        tok, lp = run_sampler(native, np.stack(cv), np.stack(ci), _params(t), L)
        check_rows(tok, lp, ref, "exact/%s" % L)


def test_edges(native):
    failures = []
    for e in S.edges():
        ref = S.sample_ref(e["cv"], e["ci"], e["T"], e["top_k"], e["top_p"], e["seed"], e["step"])
        assert not ref[3], e["name"]  # no edge is ambiguous
        p = dict(T=np.array([e["T"]], dtype=np.float32), top_k=np.array([e["top_k"]], dtype=np.int32),
                 top_p=np.array([e["top_p"]], dtype=np.float32), seed=np.array([e["seed"]], dtype=np.int64),
                 step=np.array([e["step"]], dtype=np.int32))
        for L in e["list_lens"]:
            cv, ci = S.shape_lists(e["cv"], e["ci"], L or 8)
            tok, lp = run_sampler(native, cv[None], ci[None], p, L)
            ok = tok[0] == ref[0] and (abs(lp[0] - ref[1]) <= ref[2] if ref[2] > 0 else lp[0] == ref[1])
            if "token" in e:
                ok = ok and tok[0] == e["token"]
            if "logprob" in e:
                ok = ok and lp[0] == e["logprob"]
            if not ok:
                failures.append((e["name"], L, int(tok[0]), float(lp[0]), ref[:3]))
    assert not failures, failures


@pytest.mark.parametrize("which", ["by_step", "by_seed"])
def test_steps_and_seeds_move_the_draw(native, which):
    t = S.steps_tables()[which]
    ref = S.ref_rows(t["cv"], t["ci"], t["T"], t["top_k"], t["top_p"], t["seed"], t["step"])
    assert len(set(ref[0].tolist())) >= 8
    tok, lp = run_sampler(native, t["cv"], t["ci"], _params(t), t["list_len"])
    share, _ = check_rows(tok, lp, ref, "steps/" + which)
    assert share <= AMBIGUOUS_CAP


# ----------------------------------------------------------------------------- the candidate top-k
def run_topk(native, x, case):
    """cand_v, cand_i [B, chunks * K] on the CPU from one launch over strided logits, inside sentinel frames."""
    B, V = x.shape
    K, chunks, ld = case["K"], case["chunks"], case["ld"]
    buf = torch.full((B, ld), GAP, device=DEV)
    buf[:, :V] = torch.from_numpy(x).to(DEV)
    before = buf.clone()
    vbuf, cv = _framed((B, chunks * K), torch.float32, 5.5, -7.0)
    ibuf, ci = _framed((B, chunks * K), torch.int32, S.SENT_TOK, -777)
    native.topk_candidates(buf[:, :V], K, vocab_offset=case["vocab_offset"], chunks=chunks, cand_v=cv, cand_i=ci)
    torch.cuda.synchronize()
    assert _pads_intact(vbuf, -7.0) and _pads_intact(ibuf, -777) and torch.equal(buf, before)
    return cv.cpu().numpy(), ci.cpu().numpy()


@pytest.mark.parametrize("name,case", S.topk_cases(), ids=[n for n, _ in S.topk_cases()])
def test_topk_lists_exact(native, name, case):
    """Every chunk's list equals topk_ref of its slice: values and ids, ties lowest id first, (-inf, -1) past
    min(K, slice width), an empty chunk all padding; two launches give identical bits. One row per content."""
    x = S.topk_rows(case)
    V, K, chunks, off = case["V"], case["K"], case["chunks"], case["vocab_offset"]
    assert S.topk_kernel(V, chunks, K) == case["kernel"]
    cv, ci = run_topk(native, x, case)
    cv2, ci2 = run_topk(native, x, case)
    want_v, want_i = S.topk_lists_ref(x, chunks, K, off)
    Vc = S.chunk_width(V, chunks)
    for b, kind in enumerate(S.CONTENTS):
        gv, gi = cv[b], ci[b]
        assert np.array_equal(gv.view(np.uint32), cv2[b].view(np.uint32)) and np.array_equal(gi, ci2[b]), kind
        assert np.array_equal(gv, want_v[b]), (kind, np.nonzero(gv != want_v[b])[0][:8])  # float equality
        if kind != "zeros":
            bad = np.nonzero(gi != want_i[b])[0]
            assert bad.size == 0, (kind, bad[:8], gi[bad[:8]], want_i[b][bad[:8]])
            continue
        # zeros of either sign tie as values but not as radix keys: which of them are taken is not pinned. Every
        # other id is; the zeros taken are distinct zeros of the chunk
        z = (want_v[b] == 0) & (want_i[b] >= 0)
        assert np.array_equal(gi[~z], want_i[b][~z])
        for c in range(chunks):
            ids = gi[c * K:(c + 1) * K][z[c * K:(c + 1) * K]] - off
            assert len(set(ids.tolist())) == ids.size
            assert ((ids >= min(c * Vc, V)) & (ids < min((c + 1) * Vc, V))).all() and (x[b, ids] == 0).all()


@pytest.mark.parametrize("name,V,chunks,K,kmax", S.END_TO_END, ids=[e[0] for e in S.END_TO_END])
def test_end_to_end(native, name, V, chunks, K, kmax):
    """topk_candidates, then sample_candidates(list_len=K), against sample_ref over topk_ref lists of the same
    logits: one table per top-k kernel and merge route."""
    x, p = S.end_to_end_table(V, chunks, K, kmax)
    want_v, want_i = S.topk_lists_ref(x, chunks, K)
    ref = S.ref_rows(want_v, want_i, p["T"], p["top_k"], p["top_p"], p["seed"], p["step"])
    cv, ci = native.topk_candidates(torch.from_numpy(x).to(DEV), K, chunks=chunks)
    assert np.array_equal(ci.cpu().numpy(), want_i) and np.array_equal(cv.cpu().numpy(), want_v)
    tok, lp = run_sampler(native, cv.cpu().numpy(), ci.cpu().numpy(), p, K)
    share, _ = check_rows(tok, lp, ref, "end-to-end/" + name)
    assert share <= AMBIGUOUS_CAP
