"""Shared fixtures of the reranking tests (CPU and GPU): the two tiny synthetic cross-encoder checkpoints,
their fp32 transformers oracle, token-level pairs for the model tests and the rerank_select case table."""
import atexit
import functools
import json
import math
import os
import shutil
import tempfile

import numpy as np
import torch

from rag_llm_k8s_amd.models import encoder as E
from rag_llm_k8s_amd.utils import synthetic as S

FLT_MAX = float(np.finfo(np.float32).max)
MAX_LEN = 64
# bf16 weights and activations vs fp32 transformers: the bound of tests/test_encoder_cpu.py
E_BOUND = 5e-2
# (kind, hidden, heads): head sizes 32 and 64, the two the encoder attention serves
MODELS = [("bert", 384, 12), ("bert", 128, 2), ("xlm-roberta", 384, 12), ("xlm-roberta", 128, 2)]
# head_scale per model: a 0.02-std head gives nearly constant scores; these put the spread of the fp32 scores
# over the test pairs above 0.5 (asserted in the tests, on the fp32 scores alone) and no higher than needed
HEAD_SCALE = {("bert", 384): 1.5, ("bert", 128): 3.0, ("xlm-roberta", 384): 2.0, ("xlm-roberta", 128): 3.0}
ENC_STD = 0.1  # encoder matrices wide enough that the layers do visible work (test_encoder_cpu uses 0.08)
VOCAB = 1024


def word_model(kind):
    return S.WordModel(n_words=5000, seed=7 if kind == "bert" else 11)


def encoder_config(kind, H, heads):
    if kind == "bert":
        return E.EncoderConfig(vocab_size=VOCAB, hidden_size=H, num_hidden_layers=2, num_attention_heads=heads,
                               intermediate_size=2 * H, max_position_embeddings=MAX_LEN)
    return E.EncoderConfig(model_type="xlm-roberta", vocab_size=VOCAB, hidden_size=H, num_hidden_layers=2,
                           num_attention_heads=heads, intermediate_size=2 * H, max_position_embeddings=MAX_LEN + 2,
                           type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1)


def write_wordpiece_tokenizer(out_dir, wm):
    """A BERT tokenizer.json with a vocabulary laid out by rule -- specials, letters, ## letters, then the word
    model's most frequent words -- in the format train_wordpiece_tokenizer writes. The WordPiece trainer breaks
    ties in hash order, so a trained vocabulary (and every score computed from its ids) changes from run to run."""
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors

    letters = "abcdefghijklmnopqrstuvwxyz"
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(".,?!'") + list(letters) + ["##" + c for c in letters]
    seen = set(toks)
    for w in wm.words:
        if len(toks) == VOCAB:
            break
        if w not in seen:
            seen.add(w)
            toks.append(w)
    tok = Tokenizer(models.WordPiece(vocab={t: i for i, t in enumerate(toks)}, unk_token="[UNK]",
                                     max_input_chars_per_word=100))
    tok.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None,
                                                lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.decoder = decoders.WordPiece(prefix="##")
    tok.add_special_tokens(toks[:5])
    tok.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1", special_tokens=[("[CLS]", 2), ("[SEP]", 3)])
    os.makedirs(out_dir, exist_ok=True)
    tok.save(os.path.join(out_dir, "tokenizer.json"))
    with open(os.path.join(out_dir, "tokenizer_config.json"), "w") as f:
        json.dump({"cls_token": "[CLS]", "sep_token": "[SEP]", "pad_token": "[PAD]", "unk_token": "[UNK]",
                   "do_lower_case": True, "model_max_length": 512}, f)


def train_tokenizer(out_dir, kind):
    """A small tokenizer of the checkpoint's family (seconds, not the full-size training run)."""
    if kind == "bert":
        write_wordpiece_tokenizer(out_dir, word_model(kind))
    else:
        S.train_xlmr_unigram_tokenizer(out_dir, word_model(kind), corpus_words=50_000, vocab=VOCAB - 24)


@functools.lru_cache(maxsize=None)
def checkpoint(kind, H, heads):
    """Directory of the synthetic *ForSequenceClassification checkpoint (written once per process)."""
    root = tempfile.mkdtemp(prefix="rerank_ckpt_")
    atexit.register(shutil.rmtree, root, ignore_errors=True)
    d = os.path.join(root, "%s_%d" % (kind, H))
    train_tokenizer(d, kind)
    S.write_cross_encoder_checkpoint(d, encoder_config(kind, H, heads), seed=1, head_scale=HEAD_SCALE[kind, H], std=ENC_STD)
    return d


def load_model(path, device):
    with open(os.path.join(path, "config.json")) as f:
        cfg = E.EncoderConfig.from_dict(json.load(f), pooling="cls")
    return E.EncoderModel(cfg, E.EncoderWeights.from_dir(cfg, path, device), device)


def load_reranker(path, device, **kw):
    from rag_llm_k8s_amd.engine.rerank_engine import Reranker
    from rag_llm_k8s_amd.runtime.tokenizer import Tokenizer

    kw.setdefault("max_len", MAX_LEN)
    return Reranker(load_model(path, device), Tokenizer(path), **kw)


@functools.lru_cache(maxsize=None)
def hf_model(path):
    import transformers

    with open(os.path.join(path, "config.json")) as f:
        arch = json.load(f)["architectures"][0]
    m = getattr(transformers, arch).from_pretrained(path, torch_dtype=torch.float32).eval()
    m.config._attn_implementation = "eager"
    return m


def hf_scores(path, pairs):
    """fp32 transformers scores of (ids, type_ids) pairs, one unpadded sequence at a time."""
    m = hf_model(path)
    typed = m.config.type_vocab_size > 1
    out = []
    with torch.no_grad():
        for ids, types in pairs:
            kw = {"input_ids": torch.from_numpy(np.asarray(ids, dtype=np.int64))[None]}
            if typed:
                kw["token_type_ids"] = torch.from_numpy(np.asarray(types, dtype=np.int64))[None]
            out.append(float(m(**kw).logits.float()[0, 0]))
    return np.array(out, dtype=np.float64)


PAIR_LENS = (0, 5, 8, 13, 16, 17, 24, 31, 33, 48, MAX_LEN - 1, MAX_LEN)  # 0: the shortest pair the layout allows


N_DRAWS = 24  # random candidates per length


@functools.lru_cache(maxsize=None)
def token_pairs(path, seed=5):
    """12 (ids, type_ids) pairs of total lengths `specials` (3 for BERT) ... MAX_LEN, with their fp32
    transformers scores. The ordering checks need adjacent fp32 scores well apart, which 12 random pairs are
    not: each length draws N_DRAWS random bodies and keeps the one whose fp32 score lies farthest from the
    scores already kept (greedy max-min spacing). The choice looks at the fp32 oracle only, never at the code
    under test."""
    from rag_llm_k8s_amd.engine.rerank_engine import PairLayout

    with open(os.path.join(path, "tokenizer.json"), encoding="utf-8") as f:
        layout = PairLayout.from_spec(json.load(f), lambda t: None)
    rng = np.random.default_rng(seed)
    draws = []
    for L in PAIR_LENS:
        body = max(0, L - layout.specials)
        nq = min(body // 3, 9)
        cands = [layout.build(rng.integers(5, VOCAB - 30, nq).astype(np.int32),
                              rng.integers(5, VOCAB - 30, body - nq).astype(np.int32))
                 for _ in range(N_DRAWS if body else 1)]
        draws.append((cands, hf_scores(path, cands)))
    pick = {}
    for i in sorted(range(len(draws)), key=lambda i: np.ptp(draws[i][1])):  # the least free lengths choose first
        s = draws[i][1]
        taken = [draws[k][1][j] for k, j in pick.items()]
        pick[i] = int(np.argmax([min([abs(x - t) for t in taken], default=0.0) for x in s]))
    return [draws[i][0][pick[i]] for i in range(len(draws))], np.array([draws[i][1][pick[i]] for i in range(len(draws))])


def pack(pairs, device, typed, order=None):
    """(ids, lens, type_ids) of the pairs packed in `order` (default: as given -- lengths not sorted)."""
    order = list(range(len(pairs))) if order is None else order
    ids = torch.from_numpy(np.concatenate([pairs[i][0] for i in order])).to(device)
    types = torch.from_numpy(np.concatenate([pairs[i][1] for i in order])).to(device) if typed else None
    return ids, [len(pairs[i][0]) for i in order], types


def ordering_gaps(ref, e):
    """Adjacent pairs of the descending fp32 order whose gap exceeds 4 e: [(better, worse)] and the count of
    all adjacent pairs."""
    order = np.argsort(-ref, kind="stable")
    gaps = [(int(a), int(b)) for a, b in zip(order[:-1], order[1:]) if ref[a] - ref[b] > 4 * e]
    return gaps, len(order) - 1


# ---- rerank_select -----------------------------------------------------------------------------------
SELECT_SHAPES = [(Q, N, k) for Q in (1, 3) for N in (1, 5, 32, 64) for k in sorted({1, min(4, N), N})]


def select_case(Q, N, seed=0):
    """scores with ties, NaN and -inf, int64 ids beyond 2^31, ragged n_valid including 0, 1 and N."""
    rng = np.random.default_rng(seed + 31 * Q + N)
    s = rng.integers(-3, 4, (Q, N)).astype(np.float32) / 2  # few distinct values: many ties
    s[rng.random((Q, N)) < 0.15] = np.nan
    s[rng.random((Q, N)) < 0.15] = -np.inf
    s[rng.random((Q, N)) < 0.05] = np.inf
    ids = rng.integers(0, 2 ** 40, (Q, N)).astype(np.int64)
    dist = np.sort(rng.random((Q, N)).astype(np.float32), axis=1)
    nv = np.array([N, 0, min(1, N)][:Q] if Q > 1 else [N], dtype=np.int32)
    if Q == 3 and N > 2:
        nv[2] = N - 2
    return torch.from_numpy(s), torch.from_numpy(ids), torch.from_numpy(dist), torch.from_numpy(nv)


def select_oracle(scores, ids, dist, nv, k):
    """Independent reference: Python's stable sort on (is NaN, -score)."""
    Q, N = scores.shape
    oi = torch.full((Q, k), -1, dtype=torch.int64)
    od = torch.full((Q, k), FLT_MAX, dtype=torch.float32)
    os_ = torch.full((Q, k), -FLT_MAX, dtype=torch.float32)
    for q in range(Q):
        n = int(nv[q])
        s = [float(x) for x in scores[q, :n]]
        order = sorted(range(n), key=lambda i: (1, 0.0) if math.isnan(s[i]) else (0, -s[i]))
        for r, c in enumerate(order[:k]):
            oi[q, r], od[q, r], os_[q, r] = ids[q, c], dist[q, c], scores[q, c]
    return oi, od, os_


def bits_equal(a, b):
    """torch.equal on the bit patterns (NaN scores are copied, and NaN != NaN)."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)
