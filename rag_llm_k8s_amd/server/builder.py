"""Assemble a RagService from a RagConfig (the reference's module-scope init, rag.py:13-33,199-204).

Model directory = the reference's /models PVC layout (download_model.py file list). The
generator architecture is read from config.json (llama or gpt2); the embedder from
EMBED_MODEL (a local sentence-transformers directory: the reference fetched BAAI/bge-m3
from the network at startup, /root/reference/llm/rag.py:33, which is dropped here).
"""
from __future__ import annotations

import json
import logging
import os

import torch

from ..ops.fp8 import kv_cache_dtype_name, kv_cache_torch_dtype

log = logging.getLogger(__name__)


def _load_json(p, default=None):
    if os.path.exists(p):
        with open(p) as f:
            return json.load(f)
    return default


def kv_blocks_for(model, cfg, device):
    if cfg.kv_cache_blocks > 0:
        return cfg.kv_cache_blocks
    per = model.kv_bytes_per_block(kv_cache_torch_dtype(cfg.kv_cache_dtype))  # fp8: D + 4 bytes per cached row
    if torch.device(device).type == "cuda":
        free, _ = torch.cuda.mem_get_info(torch.device(device))
        budget = int(free * cfg.kv_cache_fraction)
    else:
        budget = 2 << 30
    need = cfg.max_batch * (-(-cfg.max_model_len // 64)) + 8
    return max(16, min(need, budget // per))


def build_generator(cfg, device, tp_rank=0, tp_size=1, comm=None, tp_group=None):
    from ..engine.llm_engine import LLMEngine
    from ..runtime.tokenizer import Tokenizer

    mcfg = _load_json(os.path.join(cfg.model_path, "config.json"))
    if mcfg is None:
        raise FileNotFoundError("no config.json under MODEL_PATH=%s" % cfg.model_path)
    if cfg.dtype == "mxfp4" and mcfg.get("model_type", "llama") == "gpt2":
        raise ValueError("DTYPE=mxfp4 covers Llama-family checkpoints only; this GPT-2 checkpoint serves DTYPE=bf16")
    gen = _load_json(os.path.join(cfg.model_path, "generation_config.json"), {})
    tok = Tokenizer(cfg.model_path)
    mt = mcfg.get("model_type", "llama")
    if mt == "gpt2":
        from ..models.gpt2 import GPT2Config, GPT2Model, GPT2Weights

        c = GPT2Config.from_dict(mcfg)
        w = GPT2Weights.from_checkpoint(cfg.model_path, c, device)
        model = GPT2Model(c, w, device)
        max_len = min(cfg.max_model_len, c.n_positions)
        eos = [c.eos_token_id]
    else:
        from ..models.llama import LlamaConfig, LlamaModel, LlamaWeights

        c = LlamaConfig.from_dict(mcfg)
        w = LlamaWeights.from_checkpoint(cfg.model_path, c, device, tp_rank, tp_size)
        if cfg.dtype == "fp8":  # DTYPE=fp8: e4m3fn linear weights, per-row scales (BASELINE config 5)
            w.quantize_fp8()
        elif cfg.dtype == "mxfp4":  # DTYPE=mxfp4: OCP MXFP4 linear weights, applied to this rank's shard (opt-in, lossy)
            w.quantize_mxfp4()
            if torch.device(device).type == "cuda":
                torch.cuda.empty_cache()  # hand the bf16 originals back before kv_blocks_for reads the free HBM
        max_len = min(cfg.max_model_len, c.max_position_embeddings)
        model = LlamaModel(c, w, device, comm=comm, max_positions=max_len)
        eos = c.eos_token_id
    geos = gen.get("eos_token_id", eos)
    eos = geos if isinstance(geos, list) else [geos]
    cfg.max_model_len = max_len
    blocks = kv_blocks_for(model, cfg, device)
    kv_dtype = kv_cache_dtype_name(cfg.kv_cache_dtype)
    engine = LLMEngine(model, num_blocks=blocks, max_batch=cfg.max_batch, max_prefill_tokens=cfg.max_prefill_tokens,
                       max_model_len=max_len, eos_ids=eos, use_graphs=cfg.use_cuda_graphs, tp_group=tp_group,
                       mixed_prefill_tokens=cfg.mixed_prefill_tokens, kv_dtype=kv_dtype)
    log.info("KV cache: dtype %s, %d blocks of 64 tokens, %.1f MiB", kv_dtype, blocks,
             blocks * model.kv_bytes_per_block(kv_cache_torch_dtype(kv_dtype)) / 2 ** 20)
    return engine, tok, gen


def build_embedder(cfg, device):
    from ..engine.encoder_engine import EmbeddingEngine
    from ..models.encoder import EncoderConfig, EncoderModel, EncoderWeights
    from ..runtime.tokenizer import Tokenizer

    path = cfg.embed_model
    if not os.path.isdir(path):
        raise FileNotFoundError("EMBED_MODEL=%s is not a local sentence-transformers directory (the framework "
                                "never downloads at startup; see llm/download_model.py --embedder)" % path)
    ec = EncoderConfig.from_dir(path)
    ec.max_seq_length = min(ec.max_seq_length, cfg.max_embed_len)
    w = EncoderWeights.from_dir(ec, path, device)
    return EmbeddingEngine(EncoderModel(ec, w, device), Tokenizer(path), max_batch_tokens=cfg.embed_batch_tokens)


def build_reranker(cfg, device):
    """RERANK_MODEL: a local cross-encoder directory (config.json, model.safetensors, tokenizer.json of a BERT /
    XLM-R *ForSequenceClassification checkpoint with one label). Empty = no second stage."""
    if not cfg.rerank_model:
        return None
    from ..engine.rerank_engine import Reranker
    from ..models.encoder import EncoderConfig, EncoderModel, EncoderWeights
    from ..runtime.tokenizer import Tokenizer

    cfg.validate_rerank()
    path = cfg.rerank_model
    if not os.path.isdir(path):
        raise FileNotFoundError("RERANK_MODEL=%s is not a local model directory (the framework never downloads "
                                "at startup)" % path)
    mcfg = _load_json(os.path.join(path, "config.json"))
    if mcfg is None:
        raise FileNotFoundError("no config.json under RERANK_MODEL=%s" % path)
    labels = mcfg.get("num_labels", len(mcfg["id2label"]) if mcfg.get("id2label") else 1)
    if labels != 1:
        raise ValueError("RERANK_MODEL=%s has num_labels=%d; a reranker gives one relevance score" % (path, labels))
    ec = EncoderConfig.from_dict(mcfg, pooling="cls")
    w = EncoderWeights.from_dir(ec, path, device)
    if w.head is None:
        raise ValueError("RERANK_MODEL=%s has no sequence-classification head (classifier.* tensors)" % path)
    rr = Reranker(EncoderModel(ec, w, device), Tokenizer(path), max_len=cfg.rerank_max_len,
                  max_batch_tokens=cfg.rerank_batch_tokens)
    log.info("Reranker loaded from %s: %d candidates -> %d, pairs of up to %d tokens", path, cfg.rerank_candidates,
             cfg.retrieve_k, rr.max_len)
    return rr


def build_service(cfg, start_threads=True, tp_rank=0, tp_size=1, comm=None, tp_group=None, control=None):
    from ..index.store import DocumentStore
    from .rag_service import RagService

    device = cfg.resolved_device()
    if device.startswith("cuda"):
        device = "cuda:%d" % torch.cuda.current_device() if device == "cuda" else device
    log.info("Loading model from: %s (device %s, tp %d/%d)", cfg.model_path, device, tp_rank, tp_size)
    engine, tok, gen = build_generator(cfg, device, tp_rank, tp_size, comm, tp_group)
    log.info("Model and tokenizer loaded successfully")
    embedder = build_embedder(cfg, device)
    shard = None
    cfg.validate_hybrid()  # refuses HYBRID_SEARCH=rrf with INDEX_SHARDED before anything is loaded into the store
    if cfg.index_sharded and tp_size > 1:
        shard = (tp_group, tp_rank, tp_size)  # INDEX_SHARDED=1: row shard per TP rank (parallel/dp.py)
    store = DocumentStore(cfg.index_path, embedder.dim, device=device, index_type=cfg.index_type,
                          ivf_nlist=cfg.ivf_nlist, ivf_nprobe=cfg.ivf_nprobe, recovery=cfg.index_recovery,
                          shard=shard, lexical=cfg.hybrid, hybrid_candidates=cfg.hybrid_candidates,
                          bm25_k1=cfg.bm25_k1, bm25_b=cfg.bm25_b, rrf_k=cfg.rrf_k)
    reranker = build_reranker(cfg, device) if tp_rank == 0 else None  # like the query embedder: rank 0 retrieves
    svc = RagService(cfg, engine, tok, embedder, store, gen_config=gen, start_threads=start_threads, control=control,
                     tp_group=tp_group if tp_size > 1 else None, reranker=reranker)
    return svc
