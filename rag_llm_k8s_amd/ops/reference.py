"""Pure-torch reference implementations of every kernel in ``csrc/kernels``.

Two roles:
* numerics oracle for the GPU kernel tests (computed in fp32 on the same inputs);
* the CPU execution path (BASELINE config 1: CPU plumbing, no GPU).

Semantics follow the reference's dependencies (transformers' Llama / XLM-R / BERT /
GPT-2 modules, sentence-transformers pooling, faiss IndexFlatL2) as catalogued in
SURVEY.md §2.4.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

EPI = {"none": 0, "bias": 1, "resid": 2, "bias_resid": 3, "bias_gelu": 4, "silu_mul": 5, "gelu": 6,
       "bias_gelu_tanh": 7}


def pack_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """Pack [I,K] gate and up weights into the kernel layout: 128-row tiles of
    [64 gate rows | 64 up rows]. Requires I % 64 == 0."""
    I, K = gate.shape
    assert up.shape == gate.shape and I % 64 == 0, (gate.shape, up.shape)
    g = gate.reshape(I // 64, 64, K)
    u = up.reshape(I // 64, 64, K)
    return torch.stack([g, u], dim=1).reshape(2 * I, K).contiguous()


def unpack_gate_up(w: torch.Tensor):
    n2, K = w.shape
    t = w.reshape(n2 // 128, 2, 64, K)
    return t[:, 0].reshape(n2 // 2, K), t[:, 1].reshape(n2 // 2, K)


def linear(x, w, bias=None, resid=None, epi="none", out_f32=False):
    """C = x @ w^T with the fused epilogues of ragk_gemm (fp32 accumulate)."""
    xf = x.float()
    if epi == "silu_mul":
        g, u = unpack_gate_up(w)
        y = F.silu(xf @ g.float().t()) * (xf @ u.float().t())
    else:
        y = xf @ w.float().t()
        if bias is not None and "bias" in epi:
            y = y + bias.float()
        if resid is not None and "resid" in epi:
            y = y + resid.float()
        if epi in ("bias_gelu", "gelu"):
            y = F.gelu(y)
        elif epi == "bias_gelu_tanh":
            y = F.gelu(y, approximate="tanh")
    return y if out_f32 else y.to(x.dtype)


def rmsnorm(x, w, eps, resid=None):
    """HF LlamaRMSNorm; with resid: resid <- bf16(x + resid) first (in place)."""
    if resid is not None:
        resid.copy_((x.float() + resid.float()).to(resid.dtype))
        x = resid
    h = x.float()
    var = h.pow(2).mean(-1, keepdim=True)
    h = (h * torch.rsqrt(var + eps)).to(x.dtype)
    return (w.float() * h.float()).to(x.dtype)


def layernorm(x, g, b, eps, resid=None):
    h = x.float() if resid is None else x.float() + resid.float()
    return F.layer_norm(h, (h.shape[-1],), g.float(), b.float(), eps).to(x.dtype)


def rope_tables(head_dim, max_pos, theta=10000.0, scaling=None, dtype=torch.bfloat16):
    """cos/sin tables [max_pos, head_dim/2] (fp32 storing `dtype`-rounded values), with
    optional llama3 scaling dict {factor, low_freq_factor, high_freq_factor,
    original_max_position_embeddings} ([dep] modeling_rope_utils.py llama3 rule)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    if scaling is not None and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        low = scaling["low_freq_factor"]
        high = scaling["high_freq_factor"]
        old = scaling["original_max_position_embeddings"]
        low_wl, high_wl = old / low, old / high
        wavelen = 2 * math.pi / inv_freq
        inv_l = torch.where(wavelen > low_wl, inv_freq / factor, inv_freq)
        smooth = (old / wavelen - low) / (high - low)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        is_medium = (~(wavelen < high_wl)) & (~(wavelen > low_wl))
        inv_freq = torch.where(is_medium, smoothed, inv_l)
    pos = torch.arange(max_pos, dtype=torch.float32)
    freqs = torch.outer(pos, inv_freq.float())
    return freqs.cos().to(dtype).float().contiguous(), freqs.sin().to(dtype).float().contiguous()


def apply_rope(x, positions, cos_t, sin_t):
    """x: [T, H, D] -> rotate_half RoPE with bf16 op rounding (HF apply_rotary_pos_emb)."""
    dt = x.dtype
    c = cos_t[positions].to(dt)[:, None, :]
    s = sin_t[positions].to(dt)[:, None, :]
    c = torch.cat([c, c], -1)
    s = torch.cat([s, s], -1)
    half = x.shape[-1] // 2
    rot = torch.cat([-x[..., half:], x[..., :half]], -1)
    return (x * c) + (rot * s)


def attention_varlen(q, k, v, cu_q, kv_lens, causal, scale, cu_kv=None, k_full=None, v_full=None):
    """Reference attention over packed sequences.
    q: [Tq, Hq, D]; for each sequence s, keys are k_full(s)/v_full(s) of length kv_lens[s]
    (callables returning [L, Hkv, D]) or slices of packed k/v by cu_kv. Queries are the
    LAST q_len positions of the context."""
    Hq = q.shape[1]
    out = torch.empty_like(q)
    n = len(kv_lens)
    for s in range(n):
        q0, q1 = int(cu_q[s]), int(cu_q[s + 1])
        L = int(kv_lens[s])
        if k_full is not None:
            ks, vs = k_full(s), v_full(s)
        else:
            k0 = int(cu_kv[s])
            ks, vs = k[k0:k0 + L], v[k0:k0 + L]
        Hkv = ks.shape[1]
        rep = Hq // Hkv
        kk = ks.float().repeat_interleave(rep, dim=1).transpose(0, 1)  # [Hq, L, D]
        vv = vs.float().repeat_interleave(rep, dim=1).transpose(0, 1)
        qq = q[q0:q1].float().transpose(0, 1)  # [Hq, ql, D]
        att = (qq @ kk.transpose(1, 2)) * scale
        ql = q1 - q0
        if causal:
            qpos = torch.arange(L - ql, L)[:, None]
            kpos = torch.arange(L)[None, :]
            att = att.masked_fill(kpos > qpos, float("-inf"))
        p = att.softmax(-1)
        out[q0:q1] = (p @ vv).transpose(0, 1).to(q.dtype)
    return out


def paged_kv_view(cache, block_table, L, block_size):
    """Gather [L, Hkv, D] from a paged cache [nblocks, Hkv, BS, D]."""
    nb = (L + block_size - 1) // block_size
    blocks = cache[block_table[:nb].long()]  # [nb, Hkv, BS, D]
    return blocks.permute(0, 2, 1, 3).reshape(nb * block_size, cache.shape[1], cache.shape[3])[:L]


def pool_l2norm(hidden, cu, mode="cls", normalize=True):
    outs = []
    for b in range(len(cu) - 1):
        h = hidden[int(cu[b]):int(cu[b + 1])].float()
        if mode == "cls":
            v = h[0]
        elif mode == "mean":
            v = h.mean(0)
        else:
            v = h[-1]
        outs.append(v)
    o = torch.stack(outs)
    return F.normalize(o, p=2, dim=-1) if normalize else o


# ---- cross-encoder reranking (csrc/kernels/rerank.hip) ------------------------------------------------
SELECT_MAX_N = 64  # one wave lane per candidate; also the width of the search kernels' top lists


def embed_ln_tt(ids, pos_ids, type_ids, word, pos, type_table, g, b, eps):
    """LN(word[id] + pos[pos_id] + type_table[type_id]) in fp32, cast to the table dtype."""
    h = word[ids.long()].float() + pos[pos_ids.long()].float()
    h = h + type_table[type_ids.long()].float()
    return F.layer_norm(h, (h.shape[-1],), g.float(), b.float(), eps).to(word.dtype)


def cls_head(h, cu, w1, b1, w2, b2, dtype=torch.float32):
    """score[b] = w2 . tanh(W1 . h[cu[b]] + b1) + b2 (HF sequence-classification heads with one label)."""
    x = h[cu[:-1].long()].to(dtype)
    y = torch.tanh(x @ w1.to(dtype).t() + b1.to(dtype))
    return y @ w2.to(dtype).reshape(-1) + float(b2)


def _select_beats(sj, j, si, i):
    nj, ni = sj != sj, si != si
    if nj:
        return ni and j < i
    if ni:
        return True
    return sj > si or (sj == si and j < i)


def rerank_select(scores, cand_ids, cand_dist, n_valid, k):
    """Per query: the k best of the first n_valid candidates by score descending; ties keep the candidate
    order, NaN ranks last; slots past n_valid are (-1, FLT_MAX, -FLT_MAX). Bits of the inputs are copied."""
    import functools

    Q, N = scores.shape
    fmax = torch.finfo(torch.float32).max
    oi = torch.full((Q, k), -1, dtype=torch.int64)
    od = torch.full((Q, k), fmax, dtype=torch.float32)
    os_ = torch.full((Q, k), -fmax, dtype=torch.float32)
    sc = scores.float().cpu()
    for q in range(Q):
        nv = max(0, min(int(n_valid[q]), N))
        s = [float(x) for x in sc[q, :nv]]
        order = sorted(range(nv), key=functools.cmp_to_key(
            lambda a, b: -1 if _select_beats(s[a], a, s[b], b) else 1))
        for r, c in enumerate(order[:k]):
            oi[q, r], od[q, r], os_[q, r] = cand_ids[q, c], cand_dist[q, c], sc[q, c]
    return oi, od, os_


def sample_from_logits(logits, temperature, top_k, top_p, u=None):
    """Single-row HF-order sampler (temperature -> top-k -> top-p). Returns (kept token
    ids in descending-prob order, probabilities, pick). `u` in [0,1) draws the token."""
    x = logits.float()
    if temperature <= 0:
        return None, None, int(torch.argmax(x))
    x = x / temperature
    k = min(top_k if top_k > 0 else x.numel(), x.numel())
    vals, idx = torch.topk(x, k)
    probs = torch.softmax(vals, -1)
    cum_before = torch.cumsum(probs, 0) - probs
    keep = cum_before < top_p
    keep[0] = True
    kv, ki = vals[keep], idx[keep]
    p = torch.softmax(kv, -1)
    pick = None
    if u is not None:
        c = torch.cumsum(p, 0)
        j = int(torch.searchsorted(c, torch.tensor([u * float(c[-1])]), right=True)[0])
        pick = int(ki[min(j, len(ki) - 1)])
    return ki, p, pick


def sample_from_logits_candidates(vals, idx, temperature, top_p, u):
    """vals/idx: top-k candidates sorted descending. Applies temperature and top-p, then
    draws with uniform `u` (inverse CDF). Returns (kept ids, probs, picked id)."""
    x = vals.float() / temperature
    probs = torch.softmax(x, -1)
    cum_before = torch.cumsum(probs, 0) - probs
    keep = cum_before < top_p
    keep[0] = True
    ki = idx[keep]
    p = torch.softmax(x[keep], -1)
    c = torch.cumsum(p, 0)
    j = int(torch.searchsorted(c, torch.tensor([u * float(c[-1])]), right=True)[0])
    return ki, p, int(ki[min(j, len(ki) - 1)])


LOGITS_PROC_MAX_HIST = 32768  # history entries per row the native kernel stages (csrc/kernels/logits_proc.hip)
LOGITS_PROC_MAX_NGRAM = 8
LOGIT_BIAS_MAX = 300  # logit_bias entries per request (the width of the device bias tables)
PENALTY_GEN_MAX = 8192  # generated tokens a frequency / presence penalty may count (the kernel's LDS table)


def hist_write(ids, rows, pos, hist):
    """Token-history scatter: hist[rows[i], pos[i]] = ids[i] for every i with rows[i] >= 0 (in place)."""
    keep = rows >= 0
    hist[rows[keep].long(), pos[keep].long()] = ids[keep].to(hist.dtype)
    return hist


def repetition_penalty_row(x, seq, penalty, vocab_offset=0):
    """transformers' RepetitionPenaltyLogitsProcessor on one (shard of a) row, in place: every distinct id of
    `seq` inside [vocab_offset, vocab_offset + len(x)) gets x * p if x < 0 else x / p, once."""
    t = torch.unique(seq.long()) - vocab_offset
    t = t[(t >= 0) & (t < x.numel())]
    v = x[t]
    x[t] = torch.where(v < 0, v * penalty, v / penalty)
    return x


def logit_bias_row(x, ids, vals, vocab_offset=0):
    """logit_bias on one (shard of a) row, in place: x[id] = x[id] + bias for every (id, bias) whose id lies
    inside [vocab_offset, vocab_offset + len(x)). The ids are distinct."""
    t = ids.long() - vocab_offset
    keep = (t >= 0) & (t < x.numel())
    x[t[keep]] = x[t[keep]] + vals[keep]
    return x


def frequency_presence_row(x, gen, frequency, presence, vocab_offset=0):
    """OpenAI's frequency and presence penalties on one (shard of a) row, in place: every distinct id of the
    GENERATED tokens `gen` with count c gets (x - frequency * float(c)) - presence, three separately rounded
    fp32 operations (frequency / presence: fp32 scalars)."""
    t, c = torch.unique(gen.long(), return_counts=True)
    t = t - vocab_offset
    keep = (t >= 0) & (t < x.numel())
    t, c = t[keep], c[keep].to(torch.float32)
    v = x[t]
    v -= frequency * c
    v -= presence
    x[t] = v
    return x


def ngram_banned(seq, n):
    """transformers' NoRepeatNGramLogitsProcessor: the ids t[j+n-1] of every j in [0, L-n] whose n-1 tokens
    t[j..j+n-2] equal the last n-1 tokens of the sequence (nothing while L + 1 < n)."""
    L = seq.numel()
    if n < 1 or L < n:
        return seq[:0].long()
    if n == 1:
        return seq.long()
    win = seq.unfold(0, n, 1)  # [L-n+1, n]
    hit = (win[:, :n - 1] == seq[L - n + 1:]).all(1)
    return win[hit, n - 1].long()


def logits_process(logits, vocab_offset, ids, rows, pos, hist, penalty, ngram, ban_ids, ban_count, *, gen_start=None,
                   presence=None, frequency=None, bias_ids=None, bias_vals=None, bias_count=None, gen_bound=None):
    """History-dependent logit processors on fp32 logits [B, V] (a vocab shard starting at vocab_offset), in
    place, in transformers' order: repetition penalty, then the -inf writes of the n-gram ban and of the
    min_new_tokens ban list (ban_ids[b, :ban_count[b]]). Row b reads history row rows[b] (< 0: the row is left
    untouched) of length pos[b] + 1; with `ids` given (decode) hist[rows[b], pos[b]] = ids[b] is stored first.

    The keyword arguments (all None: the chain above, unchanged) add the OpenAI-style controls, all six together:
    logit_bias FIRST (bias_ids / bias_vals [hist rows, width], indexed by the HISTORY row, bias_count [B] entries
    of it), then the repetition penalty on the biased values, then frequency [B] and presence [B] over the
    generated tokens hist[rows[b], gen_start[b] : pos[b] + 1], then the -inf writes, which win. gen_bound: the
    caller's bound on the generated span of a row with a penalty (default PENALTY_GEN_MAX)."""
    B, V = logits.shape
    new = (gen_start, presence, frequency, bias_ids, bias_vals, bias_count)
    pen_form = any(a is not None for a in new)
    if pen_form:
        check_penalty_args(B, rows, pos, hist, gen_start, presence, frequency, bias_ids, bias_vals, bias_count,
                           gen_bound)
    for b in range(B):
        r = int(rows[b])
        if r < 0:
            continue
        p = int(pos[b])
        if ids is not None:
            hist[r, p] = ids[b]
        seq = hist[r, :p + 1]
        x = logits[b]
        if pen_form and int(bias_count[b]) > 0:
            nb = int(bias_count[b])
            logit_bias_row(x, bias_ids[r, :nb], bias_vals[r, :nb], vocab_offset)
        pen = float(penalty[b])
        if pen != 1.0:
            repetition_penalty_row(x, seq, torch.tensor(pen, dtype=torch.float32), vocab_offset)
        if pen_form and (float(presence[b]) != 0.0 or float(frequency[b]) != 0.0):
            frequency_presence_row(x, seq[int(gen_start[b]):], frequency[b].clone(), presence[b].clone(), vocab_offset)
        n = int(ngram[b])
        bans = [ngram_banned(seq, n) if n > 0 else seq[:0].long(), ban_ids[b, :int(ban_count[b])].long()]
        t = torch.cat(bans) - vocab_offset
        x[t[(t >= 0) & (t < V)]] = float("-inf")
    return logits


def check_penalty_args(B, rows, pos, hist, gen_start, presence, frequency, bias_ids, bias_vals, bias_count, gen_bound,
                       read_rows=True):
    """Host-side refusals of the penalty form of logits_process, shared by both backends (ValueError, before any
    launch): a missing argument, wrong shapes / dtypes, a bias table narrower than a row's bias_count, a gen_bound
    over PENALTY_GEN_MAX and, with read_rows (the arguments are host tensors), a gen_start outside 0..pos + 1 or
    a penalised generated span over the bound."""
    if any(a is None for a in (gen_start, presence, frequency, bias_ids, bias_vals, bias_count)):
        raise ValueError("gen_start, presence, frequency, bias_ids, bias_vals and bias_count go together")
    for t, dt, name in ((gen_start, torch.int32, "gen_start"), (bias_count, torch.int32, "bias_count"),
                        (presence, torch.float32, "presence"), (frequency, torch.float32, "frequency")):
        if t.dtype != dt or t.dim() != 1 or t.numel() != B or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s [%d] tensor" % (name, str(dt).split(".")[1], B))
    for t, dt, name in ((bias_ids, torch.int32, "bias_ids"), (bias_vals, torch.float32, "bias_vals")):
        if t.dtype != dt or t.dim() != 2 or t.shape[0] != hist.shape[0] or t.shape[1] < 1 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s [history rows = %d, width] tensor"
                             % (name, str(dt).split(".")[1], hist.shape[0]))
    if bias_ids.shape != bias_vals.shape:
        raise ValueError("bias_ids and bias_vals must have one shape")
    bound = PENALTY_GEN_MAX if gen_bound is None else int(gen_bound)
    if not 0 <= bound <= PENALTY_GEN_MAX:
        raise ValueError("a generated span of %d tokens exceeds the %d the penalties count" % (bound, PENALTY_GEN_MAX))
    if not read_rows:
        return bound
    for b in range(B):
        if int(rows[b]) < 0:
            continue
        if not 0 <= int(bias_count[b]) <= bias_ids.shape[1]:
            raise ValueError("bias_count[%d] = %d does not fit the %d-wide bias table"
                             % (b, int(bias_count[b]), bias_ids.shape[1]))
        g, p = int(gen_start[b]), int(pos[b])
        if not 0 <= g <= p + 1:
            raise ValueError("gen_start[%d] = %d outside 0..pos + 1 = %d" % (b, g, p + 1))
        if (float(presence[b]) != 0.0 or float(frequency[b]) != 0.0) and p + 1 - g > bound:
            raise ValueError("row %d: a generated span of %d tokens exceeds the bound %d" % (b, p + 1 - g, bound))
    return bound


LOGPROBS_MAX = 20  # alternatives per generated position (csrc/kernels/logprobs.hip LP_MAX)
LSE_MAX_PARTS = 512  # partials per row the finish kernel folds: 64 chunks x 8 tensor-parallel ranks
LSE_SMALL_BATCH_MAX_B = 64
LSE_SMALL_BATCH_CHUNK = 4096
LSE_CHUNK = 16384


def lse_chunks(V, B):
    """Workgroups per row of lse_partials, from the PADDED shard width V (every TP rank: the same count): ~4k
    logits each up to batch 64 (a 128k vocabulary at batch 1 spreads over 31 CUs), ~16k above; 1..64."""
    return max(1, min(V // (LSE_SMALL_BATCH_CHUNK if B <= LSE_SMALL_BATCH_MAX_B else LSE_CHUNK), 64))


def lse_chunk_width(V, chunks):
    """Entries per chunk (the candidate top-k's rule): ceil(V / chunks) rounded up to a multiple of 8."""
    return ((V + chunks - 1) // chunks + 7) & ~7


def lse_partials(logits, chunks, out=None):
    """part[b, c] = (m, s): m = max and s = sum exp(x - m) over logits[b, c * Vc : min((c + 1) * Vc, V)], fp32.
    A chunk that is empty or all -inf gives (-inf, 0)."""
    B, V = logits.shape
    if not 1 <= chunks <= 64:
        raise ValueError("1 <= chunks <= 64")
    Vc = lse_chunk_width(V, chunks)
    part = torch.empty((B, chunks, 2), dtype=torch.float32) if out is None else out
    x = logits.float()
    for c in range(chunks):
        seg = x[:, min(c * Vc, V):min((c + 1) * Vc, V)]
        if seg.shape[1] == 0:
            part[:, c, 0], part[:, c, 1] = float("-inf"), 0.0
            continue
        m = seg.max(1).values
        ok = m > float("-inf")
        s = torch.exp(seg - torch.where(ok, m, torch.zeros_like(m))[:, None]).sum(1)
        part[:, c, 0] = m
        part[:, c, 1] = torch.where(ok, s, torch.zeros_like(s))
    return part


def lse_from_partials(part):
    """lse[b] = M + log(S), M = max_p m_p, S = sum over ascending p of s_p * exp(m_p - M) (m_p = -inf adds 0)."""
    m, s = part[..., 0].float(), part[..., 1].float()
    M = m.max(1).values
    S = torch.zeros_like(M)
    for p in range(m.shape[1]):
        dead = m[:, p] == float("-inf")
        e = torch.exp(torch.where(dead, torch.zeros_like(M), m[:, p] - M))
        S = S + torch.where(dead, torch.zeros_like(M), s[:, p] * e)
    return M + torch.log(S)


def logprobs_finish(part, cand_v, cand_i, list_len, tok, nlp, out_lse=None, out_tok_lp=None, out_top_lp=None,
                    out_top_id=None):
    """Per-row log-probabilities from the lse partials [B, P, 2] and the candidate lists the sampler got
    (cand_v / cand_i [B, n] = n / list_len sorted lists): row b with N = nlp[b] >= 0 gets out_lse[b],
    out_tok_lp[b] = v_j - lse for the candidate j whose id is tok[b] (NaN if there is none) and, in slots
    0..N-1 of out_top_id / out_top_lp [B, LOGPROBS_MAX], the first N candidates by (value desc, id asc) as
    (id, v - lse). Slots >= N and rows with nlp < 0 are left untouched."""
    B, n = cand_v.shape
    if list_len < LOGPROBS_MAX or n % list_len:
        raise ValueError("logprobs_finish: candidate lists of at least %d entries" % LOGPROBS_MAX)
    if not 1 <= part.shape[1] <= LSE_MAX_PARTS:
        raise ValueError("logprobs_finish: 1..%d partials per row" % LSE_MAX_PARTS)
    nan = float("nan")
    out_lse = torch.full((B,), nan) if out_lse is None else out_lse
    out_tok_lp = torch.full((B,), nan) if out_tok_lp is None else out_tok_lp
    out_top_lp = torch.full((B, LOGPROBS_MAX), nan) if out_top_lp is None else out_top_lp
    out_top_id = torch.full((B, LOGPROBS_MAX), -1, dtype=torch.int32) if out_top_id is None else out_top_id
    lse = lse_from_partials(part)
    for b in range(B):
        N = min(int(nlp[b]), LOGPROBS_MAX)
        if N < 0:
            continue
        out_lse[b] = lse[b]
        v, i = cand_v[b].float(), cand_i[b].long()
        t = int(tok[b])
        hit = (i == t).nonzero().flatten() if t >= 0 else i[:0]
        out_tok_lp[b] = v[hit[0]] - lse[b] if hit.numel() else nan
        if N == 0:
            continue
        # only the first N of each sorted list can qualify; padding (id -1) sorts last
        head = (torch.arange(n) % list_len) < N
        hv, hi = v[head], i[head]
        hv = torch.where(hi >= 0, hv, torch.full_like(hv, float("-inf")))
        key = torch.where(hi >= 0, hi, torch.full_like(hi, 1 << 32))
        o = torch.argsort(key, stable=True)
        o = o[torch.argsort(hv[o], descending=True, stable=True)][:N]
        k = o.numel()
        out_top_id[b, :k] = hi[o].to(out_top_id.dtype)
        out_top_lp[b, :k] = hv[o] - lse[b]
    return out_lse, out_tok_lp, out_top_lp, out_top_id


def l2_knn(xb, q, k):
    """faiss IndexFlatL2.search: squared L2, ascending; pad (-1, FLT_MAX)."""
    n = xb.shape[0]
    nq = q.shape[0]
    D = torch.full((nq, k), torch.finfo(torch.float32).max)
    I = torch.full((nq, k), -1, dtype=torch.int64)
    if n == 0:
        return D, I
    d = ((q[:, None, :].double() - xb[None, :, :].double()) ** 2).sum(-1).float()
    kk = min(k, n)
    dv, di = torch.sort(d, dim=1, stable=True)
    D[:, :kk] = dv[:, :kk]
    I[:, :kk] = di[:, :kk]
    return D, I


# ----------------------------------------------------------------------------- BM25 lexical search
# fp32 replicas of csrc/kernels/lexical.hip. Layout (index/lexical.py): a doc-major CSR -- row_ptr int64 [n + 1],
# terms int32 (the uint32 term ids' bit patterns, ascending within a document), tf int16 (uint16 bit patterns),
# doc_len int32 [n]. A launch's term table: qterms int32 [T] (uint32 bit patterns, ascending as unsigned,
# distinct), idf fp32 [T], member int64 [T] (bit q set: query q holds the term).
LEX_MAX_TERMS = 4096
LEX_MAX_QUERIES = 64


def _lex_hits(row_ptr, terms, n, qterms):
    """The CSR entries whose term is in the table, in entry order: (document [h], table position [h], entry
    index [h])."""
    rp = row_ptr[:n + 1].cpu().long()
    nnz = int(rp[n]) if n else 0
    t = terms[:nnz].cpu().long() & 0xFFFFFFFF
    qt = qterms.cpu().long() & 0xFFFFFFFF
    T = qt.numel()
    if T == 0 or nnz == 0:
        z = torch.zeros(0, dtype=torch.int64)
        return z, z, z
    pos = torch.searchsorted(qt, t).clamp_(max=T - 1)
    hit = torch.nonzero(qt[pos] == t).reshape(-1)
    doc_of = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    return doc_of[hit], pos[hit], hit


def _lex_table_ok(qterms):
    qt = qterms.cpu().long() & 0xFFFFFFFF
    if qt.numel() > LEX_MAX_TERMS:
        raise ValueError("lexical search: at most %d terms per launch" % LEX_MAX_TERMS)
    if qt.numel() > 1 and not bool((qt[1:] > qt[:-1]).all()):
        raise ValueError("lexical search: the term table must be strictly ascending (as unsigned ids)")


def _lex_allowed(masks, qmask, n):
    from ..index.flat import mask_allowed

    return torch.from_numpy(mask_allowed(masks, qmask, torch.arange(n).numpy()))


def lex_df(row_ptr, terms, n, qterms, live=None):
    """int32 [T]: the documents among the first n -- those whose bit is set in the bitmap row `live` (uint32 /
    int32 words), or all of them -- that hold each table term."""
    _lex_table_ok(qterms)
    T = qterms.numel()
    hd, ht, _ = _lex_hits(row_ptr, terms, n, qterms)
    if live is not None and hd.numel():
        lv = live.cpu() if isinstance(live, torch.Tensor) else live
        ok = _lex_allowed(lv.reshape(1, -1), torch.zeros(1, dtype=torch.int32), n)[0]
        ht = ht[ok[hd]]
    return torch.bincount(ht, minlength=T).to(torch.int32)


def lex_search(row_ptr, terms, tf, doc_len, n, qterms, idf, member, nq, k1, k1p1, b, avgdl, k, masks=None,
               qmask=None):
    """Top k documents per query by BM25 -> (scores fp32 [nq, k] descending, ids int64 [nq, k], ties -> lower id,
    padding (0, -1)). The kernel's arithmetic, every operation rounded to fp32 on its own:
        norm = k1 * ((1 - b) + b * (float(dl) / avgdl));  c = idf * ((float(tf) * k1p1) / (float(tf) + norm))
    and a document's score is the sum of its matching terms' c in ascending term-id (= entry) order. A document
    with no matching term is no candidate. masks / qmask: per-query id bitmaps as in the L2 search."""
    _lex_table_ok(qterms)
    if not 1 <= k <= 64 or not 0 <= nq <= LEX_MAX_QUERIES:
        raise ValueError("lexical search: 1 <= k <= 64 and at most %d queries per launch" % LEX_MAX_QUERIES)
    f32 = torch.float32
    S = torch.zeros((nq, k), dtype=f32)
    I = torch.full((nq, k), -1, dtype=torch.int64)
    hd, ht, he = _lex_hits(row_ptr, terms, n, qterms)
    if nq == 0 or hd.numel() == 0:
        return S, I
    k1, k1p1, b, avgdl = (torch.tensor(float(v), dtype=f32) for v in (k1, k1p1, b, avgdl))
    ftf = (tf.cpu().long()[he] & 0xFFFF).to(f32)
    dl = doc_len[:n].cpu().to(f32)
    norm = k1 * ((torch.tensor(1.0, dtype=f32) - b) + b * (dl / avgdl))
    c = idf.cpu().to(f32)[ht] * ((ftf * k1p1) / (ftf + norm[hd]))
    bits = ((member.cpu().long()[ht].unsqueeze(1) >> torch.arange(nq)) & 1).bool()  # [hits, nq]
    cnt = torch.bincount(hd, minlength=n)
    rank = torch.arange(hd.numel()) - (torch.cumsum(cnt, 0) - cnt)[hd]  # a hit's place among its document's hits
    order = torch.argsort(rank, stable=True)
    per_rank = torch.bincount(rank).tolist()
    score = torch.zeros((n, nq), dtype=f32)
    matched = torch.zeros((n, nq), dtype=torch.bool)
    zero = torch.zeros((), dtype=f32)
    o0 = 0
    for m in per_rank:  # the r-th hit of every document at once: one document per row, so the adds stay ordered
        sel = order[o0:o0 + m]
        o0 += m
        d = hd[sel]
        score[d] = score[d] + torch.where(bits[sel], c[sel].unsqueeze(1), zero)  # x + 0 == x: non-members keep theirs
        matched[d] |= bits[sel]
    cand = matched.t()
    if masks is not None or qmask is not None:
        mk = masks.cpu() if isinstance(masks, torch.Tensor) else masks
        qm = qmask.cpu() if isinstance(qmask, torch.Tensor) else qmask
        cand = cand & _lex_allowed(mk, qm, n)
    key = torch.where(cand, -score.t(), torch.full((), float("inf"), dtype=f32))
    kv, ki = torch.sort(key, dim=1, stable=True)  # ascending -score; equal scores keep ascending ids
    kk = min(k, n)
    ok = kv[:, :kk] != float("inf")
    S[:, :kk] = torch.where(ok, -kv[:, :kk], S[:, :kk])
    I[:, :kk] = torch.where(ok, ki[:, :kk], I[:, :kk])
    return S, I
