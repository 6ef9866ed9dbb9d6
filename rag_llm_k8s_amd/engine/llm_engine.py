"""Continuous-batching generation engine (replaces transformers' generate loop, D2).

Reference loop ([dep] generation/utils.py _sample, driven from /root/reference/llm/rag.py:172):
one prompt at a time, DynamicCache, temperature -> top-k(50) -> top-p -> multinomial, stop on
EOS or max_new_tokens. The reference runs concurrent Flask requests as independent
generate() calls with no batching.

Here:
  * requests join a waiting queue; each engine step is either a PREFILL step (new prompts,
    packed varlen, chunked to `max_prefill_tokens`) or a DECODE step over every running
    sequence (continuous batching: sequences enter/leave between steps);
  * KV lives in a paged cache (64-token blocks, block manager); admission reserves the
    blocks for prompt + max_new_tokens, so a running sequence is never preempted;
  * decode steps replay a hipGraph per batch-size bucket (static input buffers, one H2D
    copy of a packed metadata block, sampling inside the graph); the host only reads back
    the sampled token ids;
  * tensor parallel: every TP rank runs the same deterministic schedule on the same inputs
    (rank 0 broadcasts new requests), so no per-step metadata broadcast is needed.
"""
from __future__ import annotations

import gc
import itertools
import logging
import math
import os
import threading
import time
from collections import deque
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from ..models.llama import StepInput
from ..ops.backend import AttnMeta
from ..ops.fp8 import kv_cache_dtype_name, kv_cache_torch_dtype
# per-token log-probabilities (csrc/kernels/logprobs.hip): LOGPROBS_MAX = most alternatives per position
from ..ops.reference import LOGPROBS_MAX, lse_chunks
# logit_bias entries per request, and the most tokens a request with a frequency / presence penalty may generate
# (the LDS counting table of csrc/kernels/logits_proc.hip)
from ..ops.reference import LOGIT_BIAS_MAX, PENALTY_GEN_MAX
from ..utils import faults
from .kv_manager import BLOCK, make_block_manager
from .step_layout import BAN_IDS_MAX, StepLayout, graph_key

# decode batches up to this size split each row's top-k over ~31 chunks of ~4k logits (topk_wave_kernel,
# threshold-filtered lane networks, merged by the sampler's lane network); larger batches use 7
# radix-select chunks (topk_lds). tools/sampler_bench.py: top-k + sample 21.0 us at batch 1 (7 chunks:
# 40.1), 33.6 us at batch 32 (7 chunks: 41.2) -- profiles/sampler_bench_r3.log
SMALL_BATCH_TOPK_MAX_B = 64
SMALL_BATCH_TOPK_CHUNK = 4096

# history-dependent logit processors (csrc/kernels/logits_proc.hip): widest n-gram ban
NGRAM_MAX = 8

log = logging.getLogger(__name__)


@dataclass
class SamplingParams:
    max_new_tokens: int = 150
    temperature: float = 0.7
    top_p: float = 0.9
    top_k: int = 50
    do_sample: bool = True
    seed: Optional[int] = None
    stop_token_ids: tuple = ()
    ignore_eos: bool = False  # benchmark mode: always generate max_new_tokens
    # history-dependent logit processors, transformers' semantics over prompt + generated tokens; the
    # defaults mean off, and a request that enables none runs exactly the launches it ran without them
    repetition_penalty: float = 1.0  # RepetitionPenaltyLogitsProcessor
    no_repeat_ngram_size: int = 0  # NoRepeatNGramLogitsProcessor, 0..NGRAM_MAX
    min_new_tokens: int = 0  # MinNewTokensLengthLogitsProcessor over eos + stop_token_ids
    # None = off; N in 0..LOGPROBS_MAX: every generated token's log-probability plus the N most likely
    # alternatives, log_softmax of the fp32 logits after the processors above and before temperature / top-k /
    # top-p (transformers' `scores` of a greedy generate; the unwarped model distribution for sampled requests)
    logprobs: Optional[int] = None
    # OpenAI-style controls, applied with the processors above (ops/reference.py logits_process): logit_bias
    # first, then the repetition penalty, then frequency and presence over the GENERATED tokens only
    # (x - frequency * count - presence for every generated id), then the -inf bans. 0.0 / () mean off.
    presence_penalty: float = 0.0  # -2..2
    frequency_penalty: float = 0.0  # -2..2
    logit_bias: tuple = ()  # ((token id, bias in -100..100), ...) sorted by id, at most LOGIT_BIAS_MAX

    def uses_penalties(self) -> bool:
        return self.presence_penalty != 0.0 or self.frequency_penalty != 0.0 or len(self.logit_bias) > 0

    def uses_processors(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0
                or (self.min_new_tokens > 0 and not self.ignore_eos) or self.uses_penalties())


def normalize_logit_bias(bias) -> tuple:
    """SamplingParams.logit_bias from a mapping {id: bias} or an iterable of (id, bias) pairs: a tuple of
    (int id, float bias) sorted by id. Raises ValueError for an id that is not an integer, a value that is not a
    number, or a duplicate id; ranges are check_params' business."""
    items = list(bias.items()) if hasattr(bias, "items") else [tuple(e) for e in bias]
    out = []
    for e in items:
        if len(e) != 2:
            raise ValueError("logit_bias entries are (token id, bias) pairs (got %r)" % (e,))
        t, v = e
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise ValueError("logit_bias: token id %r is not an integer" % (t,))
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("logit_bias: the bias of token %d must be a number (got %r)" % (t, v))
        out.append((int(t), float(v)))
    out.sort()
    for a, b in zip(out, out[1:]):
        if a[0] == b[0]:
            raise ValueError("logit_bias: token id %d occurs twice" % a[0])
    return tuple(out)


WAITING, RUNNING, FINISHED = 0, 1, 2


class Sequence:
    _ids = itertools.count()

    def __init__(self, prompt_ids, params: SamplingParams, seed: int):
        self.id = next(Sequence._ids)
        if isinstance(prompt_ids, np.ndarray):  # int32 buffers (TP admission broadcast)
            self.prompt_np = np.ascontiguousarray(prompt_ids, dtype=np.int32)
            self.prompt = self.prompt_np.tolist()
        else:
            self.prompt = list(prompt_ids)
            self.prompt_np = np.asarray(self.prompt, dtype=np.int32)  # vectorised prefill input building
        self.out: List[int] = []
        self.params = params
        self.seed = seed
        self.computed = 0  # tokens whose K/V is in the cache
        self.status = WAITING
        self.t_arrive = time.perf_counter()
        self.t_first = None
        self.t_done = None
        self.finish_reason = None
        self.done = threading.Event()
        self.user = None  # opaque payload for the caller
        self.hist_row = -1  # row of the engine's device token history (-1: no logit processors)
        # per generated token (len == len(out) at all times) for a request with params.logprobs, else None:
        # its log-probability, and the top-N alternatives as [(id, logprob)] by (logprob desc, id asc)
        want = getattr(params, "logprobs", None) is not None
        self.logprobs: Optional[List[float]] = [] if want else None
        self.top_logprobs: Optional[List[list]] = [] if want else None

    @property
    def length(self):
        return len(self.prompt) + len(self.out)

    def token_at(self, i):
        n = len(self.prompt)
        return self.prompt[i] if i < n else self.out[i - n]


class LLMEngine:
    def __init__(self, model, num_blocks: int, max_batch: int = 64, max_prefill_tokens: int = 32768,
                 max_model_len: int = 16384, eos_ids=(), use_graphs: bool = True, tp_group=None, top_k_cap: int = 64,
                 graph_buckets=None, mixed_prefill_tokens: int = 0, kv_dtype="bf16"):
        self.model = model
        self.device = model.device
        self.max_batch = max_batch
        self.max_prefill_tokens = max_prefill_tokens
        # Decode-aware prefill budget (served path): a step that carries decoding rows takes at most this
        # many prompt tokens, so the rows' per-token latency (TPOT) is one short step, not a whole
        # max_prefill_tokens chunk; with nothing decoding the full budget applies (TTFT, throughput).
        # 0 = off (offline batch / the headline bench: its wave is throughput-bound).
        self.mixed_prefill_tokens = int(mixed_prefill_tokens or 0)
        self.max_model_len = max_model_len
        self.eos = set(int(e) for e in eos_ids)
        self.bm = make_block_manager(num_blocks)
        self.max_blocks = -(-max_model_len // BLOCK)
        # "bf16" (default) or "fp8": e4m3 K / V with one fp32 scale per cached row (ops/fp8.Fp8KV); a model the
        # fp8 kernels do not cover (head_dim != 128, GPT-2) raises here instead of silently running bf16
        self.kv_dtype = kv_cache_dtype_name(kv_dtype)
        if self.kv_dtype == "bf16":
            model.allocate_kv_cache(num_blocks)
        else:
            model.allocate_kv_cache(num_blocks, kv_cache_torch_dtype(kv_dtype))
        self.waiting = deque()
        self.running: List[Sequence] = []
        self.lock = threading.Lock()
        self._aborts = []
        self.tp_group = tp_group
        self.comm = getattr(model, "comm", None)
        if self.comm is not None and self.comm.size > 1:
            self.tp_size = self.comm.size
        else:
            self.tp_size = 1 if tp_group is None else torch.distributed.get_world_size(tp_group)
        # candidate-list width of the native sampler (top-k <= K served inside the decode graph);
        # requests with a larger top_k, or top_k = 0 (HF: disabled), take the exact full-vocabulary path
        self.K = top_k_cap
        self._warned_topk = False
        # TP prefill steps of at least this many tokens run as 2 micro-batches with async all-reduces
        self.tp_overlap_min_tokens = 1024
        self.is_cuda = self.device.type == "cuda"
        self.use_graphs = use_graphs and self.is_cuda
        self.buckets = sorted(set(graph_buckets or [b for b in (1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 192, 256)
                                                    if b <= max_batch] + [max_batch]))
        self.graphs = {}
        # RAGK_DECODE_TIMING=1: (start, end) CUDA events around every async decode graph replay
        self._timing = [] if os.environ.get("RAGK_DECODE_TIMING") == "1" else None
        self.stats = dict(prefill_steps=0, decode_steps=0, prefill_tokens=0, decode_tokens=0, prefill_s=0.0,
                          decode_s=0.0, kv_dtype=self.kv_dtype)
        # two pinned staging buffers, alternated per step: with the asynchronous decode pipeline a
        # step's H2D copy may still be pending while the host stages the next one
        self._pins = [torch.empty(1 << 20 if self.is_cuda else 0, dtype=torch.int32, pin_memory=self.is_cuda)
                      for _ in range(2)]
        self._pin_idx = 0
        self._pin = self._pins[0]
        self._pin_off = 0
        # Asynchronous decode (hipGraph path): step t+1 is enqueued before step t's tokens are read
        # back; its input ids come from step t's sampled tokens on the device (D2D), so the GPU never
        # waits for the host round trip between decode steps. Tokens are accepted one step late; a
        # sequence that stops on EOS has computed one extra (discarded) row, and its KV blocks are
        # freed only after that step has completed. Under TP every rank samples the same token from
        # the same gathered candidates, so all ranks take the same decisions one step late.
        self.async_decode = self.use_graphs and os.environ.get("RAGK_ASYNC_DECODE", "1") == "1"
        # Mixed prefill + decode steps (chunked prefill): a step that admits prompt tokens
        # also advances every decoding sequence by one token through the same forward.
        self.mixed_steps = os.environ.get("RAGK_MIXED_STEPS", "1") == "1"
        self._inflight = None  # dict(seqs, rows, entry, event, host_out, n)
        self._free_after = []  # seq ids whose blocks are freed once the in-flight step has completed
        self._out_pins = [torch.empty(max(1, max_batch), dtype=torch.int32, pin_memory=self.is_cuda)
                          for _ in range(2)]
        self._out_idx = 0
        # sampled tokens of every decode graph land in this one device buffer: the next step's graph
        # (any bucket) reads its carried ids from it inside the embedding kernel (packed "carry" map)
        self._tok_out = torch.zeros(max(self.buckets + [max_batch, 1]), dtype=torch.int32,
                                    device=self.device) if self.is_cuda else None
        # Device token history of the logit processors: hist[row][position] = token at that position, one row
        # per sequence that enables a processor, allocated at the first such request (_ensure_hist). Every
        # write is idempotent, so discarded / recomputed steps rewrite the same cells; a finished sequence's
        # row is released with the same deferral as its KV blocks (_hist_after).
        self._hist = None
        self._hist_free = None
        self._hist_after = []
        self.stats["logit_proc_steps"] = 0
        self.stats["penalty_steps"] = 0  # of those: steps with a row that uses presence / frequency / logit_bias
        # per-token log-probabilities: steps that had a row asking for them, and the two pinned read-back
        # buffers of the asynchronous pipeline (allocated at the first such step, alternated like _out_pins)
        self.stats["logprob_steps"] = 0
        self._lp_pins = None

    # ------------------------------------------------------------------ requests
    def add_request(self, prompt_ids, params: SamplingParams, seed: Optional[int] = None) -> Sequence:
        if len(prompt_ids) == 0:
            raise ValueError("empty prompt")
        if len(prompt_ids) + params.max_new_tokens > self.max_model_len:
            raise ValueError("prompt (%d) + max_new_tokens (%d) exceeds max_model_len %d"
                             % (len(prompt_ids), params.max_new_tokens, self.max_model_len))
        self.check_params(params)
        s = Sequence(prompt_ids, params, seed if seed is not None else (params.seed if params.seed is not None
                                                                        else int(time.time_ns() & 0xFFFFFFFF)))
        with self.lock:
            self.waiting.append(s)
        return s

    def make_sequence(self, prompt_ids, params: SamplingParams, seed: int) -> Sequence:
        if len(prompt_ids) == 0:
            raise ValueError("empty prompt")
        if len(prompt_ids) + params.max_new_tokens > self.max_model_len:
            raise ValueError("prompt (%d) + max_new_tokens (%d) exceeds max_model_len %d"
                             % (len(prompt_ids), params.max_new_tokens, self.max_model_len))
        self.check_params(params)
        return Sequence(prompt_ids, params, seed)

    def _stop_ids(self, p):
        """The ids a request stops on (what min_new_tokens bans): the engine's eos set + its stop_token_ids."""
        return sorted(self.eos | set(int(t) for t in p.stop_token_ids))

    def check_params(self, p: SamplingParams):
        rp, n, m = p.repetition_penalty, p.no_repeat_ngram_size, p.min_new_tokens
        if isinstance(rp, bool) or not isinstance(rp, (int, float)) or not math.isfinite(rp) or rp <= 0:
            raise ValueError("repetition_penalty must be a finite number > 0 (got %r)" % (rp,))
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= NGRAM_MAX:
            raise ValueError("no_repeat_ngram_size must be an integer in 0..%d (got %r)" % (NGRAM_MAX, n))
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= p.max_new_tokens:
            raise ValueError("min_new_tokens must be an integer in 0..max_new_tokens=%d (got %r)"
                             % (p.max_new_tokens, m))
        if m > 0 and not p.ignore_eos and len(self._stop_ids(p)) > BAN_IDS_MAX:
            raise ValueError("min_new_tokens: at most %d eos + stop ids" % BAN_IDS_MAX)
        lp = p.logprobs
        if lp is not None:
            if isinstance(lp, bool) or not isinstance(lp, int) or not 0 <= lp <= LOGPROBS_MAX:
                raise ValueError("logprobs must be None or an integer in 0..%d (got %r)" % (LOGPROBS_MAX, lp))
            if LOGPROBS_MAX > self.K:
                raise ValueError("logprobs: the engine's candidate lists (top_k_cap = %d) are shorter than %d"
                                 % (self.K, LOGPROBS_MAX))
        for name in ("presence_penalty", "frequency_penalty"):
            v = getattr(p, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not -2 <= v <= 2:
                raise ValueError("%s must be a finite number in -2..2 (got %r)" % (name, v))
        lb = p.logit_bias
        if not isinstance(lb, tuple):
            raise ValueError("logit_bias must be a tuple of (token id, bias) pairs sorted by id (normalize_logit_bias)")
        if len(lb) > LOGIT_BIAS_MAX:
            raise ValueError("logit_bias: at most %d entries (got %d)" % (LOGIT_BIAS_MAX, len(lb)))
        if lb:
            if normalize_logit_bias(lb) != lb:
                raise ValueError("logit_bias must hold (int id, float bias) pairs sorted by id (normalize_logit_bias)")
            vocab = int(self.model.cfg.vocab_size)  # the whole vocabulary, not this rank's shard
            for t, v in lb:
                if not 0 <= t < vocab:
                    raise ValueError("logit_bias: token id %d outside the vocabulary 0..%d" % (t, vocab - 1))
                if not math.isfinite(v) or not -100 <= v <= 100:
                    raise ValueError("logit_bias: the bias of token %d must be finite, in -100..100 (got %r)" % (t, v))
        if (p.presence_penalty != 0.0 or p.frequency_penalty != 0.0) and p.max_new_tokens > PENALTY_GEN_MAX:
            raise ValueError("presence_penalty / frequency_penalty: max_new_tokens %d exceeds the %d generated "
                             "tokens the penalties count" % (p.max_new_tokens, PENALTY_GEN_MAX))
        if p.uses_processors() and self.is_cuda:
            from ..ops.native import logits_proc_max_hist
            if self.max_model_len > logits_proc_max_hist():
                raise ValueError("logit processors: max_model_len %d exceeds the %d history entries the kernel "
                                 "stages" % (self.max_model_len, logits_proc_max_hist()))

    # ------------------------------------------------------------------ token history (logit processors)
    def _ensure_hist(self):
        if self._hist is None:
            self._hist = torch.zeros((max(1, self.max_batch), self.max_model_len), dtype=torch.int32,
                                     device=self.device)
            self._hist_free = list(range(self._hist.shape[0] - 1, -1, -1))
            # logit_bias tables, one row per history row: written once when a sequence takes the row
            # (_write_bias), read by the kernel up to the row's bias count of that step's argument block
            self._bias_ids = torch.zeros((self._hist.shape[0], LOGIT_BIAS_MAX), dtype=torch.int32, device=self.device)
            self._bias_vals = torch.zeros((self._hist.shape[0], LOGIT_BIAS_MAX), dtype=torch.float32,
                                          device=self.device)

    def _write_bias(self, s):
        """The sequence's logit_bias into its history row's table row: stream-ordered copies on the compute
        stream. No in-flight step reads the row (a finished sequence's row is released only after the step that
        could still touch it has completed), and a sequence without a bias passes count 0, so nothing of the
        row's previous owner is ever read."""
        lb = s.params.logit_bias
        if not lb:
            return
        n = len(lb)
        ids = np.fromiter((t for t, _ in lb), dtype=np.int32, count=n)
        vals = np.fromiter((v for _, v in lb), dtype=np.float32, count=n)
        buf = self._h2d_i32(np.concatenate([ids, vals.view(np.int32)]))
        self._bias_ids[s.hist_row, :n].copy_(buf[:n], non_blocking=True)
        self._bias_vals[s.hist_row, :n].copy_(buf[n:].view(torch.float32), non_blocking=True)

    def _free_deferred(self):
        """The in-flight step that could still write them has completed: release the KV blocks and history
        rows of the sequences that finished while it ran."""
        for sid in self._free_after:
            self.bm.free(sid)
        self._free_after = []
        if self._hist_after:
            self._hist_free.extend(self._hist_after)
            self._hist_after = []

    def _step_key(self, seqs, full_vocab=False):
        """The graph variant (and the sections of the step block) a sampling step over `seqs` needs, counted in
        the stats. A full-vocabulary step computes its logprobs on the host: it counts as a logprob step and
        needs no logprob section."""
        proc = any(s.hist_row >= 0 for s in seqs)
        pen = any(s.hist_row >= 0 and s.params.uses_penalties() for s in seqs)
        lp = any(s.logprobs is not None for s in seqs)
        self.stats["logit_proc_steps"] += int(proc)
        self.stats["penalty_steps"] += int(pen)
        self.stats["logprob_steps"] += int(lp)
        return graph_key(self._bucket(len(seqs)), proc, lp and not full_vocab, pen)

    def _pack(self, layout, seqs, carried=None):
        return layout.pack(seqs, carried, top_k_cap=self.K, stop_ids=self._stop_ids, bt_row=self._bt_row)

    def _eager_block(self, seqs, key, max_blocks=0):
        """Views of the step block of an eager sampling call over exactly `seqs`, on the device (one H2D copy)."""
        layout = StepLayout(len(seqs), max_blocks, key.processors, key.penalties, key.logprobs)
        return layout.views(self._h2d_i32(self._pack(layout, seqs)))

    def _apply_processors(self, lg, proc):
        """proc: the views of a step block with the processor section. proc["ids"]: the step's input ids, stored
        into the history by the kernel, or None when the history is already complete (prefill's sampled rows)."""
        be = self.model.be
        if "gen_start" not in proc:
            be.logits_process(lg, self.model.w.vocab_offset, proc["ids"], proc["rows"], proc["pos"], self._hist,
                              proc["penalty"], proc["ngram"], proc["ban_ids"], proc["ban_count"])
            return
        # the penalty form. Admission bounds a penalised request's generated tokens by PENALTY_GEN_MAX; the
        # bound is a host constant, so the launch is the same at capture and at every replay
        be.logits_process(lg, self.model.w.vocab_offset, proc["ids"], proc["rows"], proc["pos"], self._hist,
                          proc["penalty"], proc["ngram"], proc["ban_ids"], proc["ban_count"],
                          gen_start=proc["gen_start"], presence=proc["presence"], frequency=proc["frequency"],
                          bias_ids=self._bias_ids, bias_vals=self._bias_vals, bias_count=proc["bias_count"],
                          gen_bound=min(PENALTY_GEN_MAX, self.max_model_len))

    # ------------------------------------------------------------------ per-token log-probabilities
    LP_WORDS = 2 + 2 * LOGPROBS_MAX  # output words per row: lse | token logprob | top logprobs | top ids

    @staticmethod
    def _lp_views(buf, n):
        """(lse [n], token logprob [n], top logprobs [n, LOGPROBS_MAX], top ids [n, LOGPROBS_MAX]) views of an
        int32 [LP_WORDS * n] buffer: one allocation, so one copy brings a step's values to the host."""
        L = LOGPROBS_MAX
        return (buf[0:n].view(torch.float32), buf[n:2 * n].view(torch.float32),
                buf[2 * n:(2 + L) * n].view(torch.float32).view(n, L), buf[(2 + L) * n:(2 + 2 * L) * n].view(n, L))

    def _lp_block(self, v, n):
        """Logprob argument block of a sampling call over the n rows of the step block views v (None without a
        logprob section): the rows' alternative counts and a fresh output buffer."""
        if "nlp" not in v:
            return None
        return dict(nlp=v["nlp"], n=n, buf=torch.zeros(self.LP_WORDS * n, dtype=torch.int32, device=self.device))

    def _lp_values(self, host, n, seqs):
        """Per sequence None or (token logprob, [(id, logprob)] of its N alternatives) from a host copy of an
        output buffer laid out for n rows (_lp_views)."""
        _, tl, tp, ti = self._lp_views(host, n)
        tl, tp, ti = tl.numpy(), tp.numpy(), ti.numpy()
        out = []
        for i, s in enumerate(seqs):
            if s.logprobs is None:
                out.append(None)
                continue
            k = s.params.logprobs
            out.append((float(tl[i]), [(int(ti[i, j]), float(tp[i, j])) for j in range(k)]))
        return out

    def _lp_pin(self, idx, words):
        if self._lp_pins is None:
            cap = self.LP_WORDS * max(self.buckets + [self.max_batch, 1])
            self._lp_pins = [torch.empty(cap, dtype=torch.int32, pin_memory=self.is_cuda) for _ in range(2)]
        return self._lp_pins[idx][:words]

    def add_sequence(self, s: Sequence):
        with self.lock:
            self.waiting.append(s)
        return s

    def has_work(self):
        return bool(self.waiting) or bool(self.running) or self._inflight is not None

    # ------------------------------------------------------------------ scheduling
    def _admit(self, reserve=0):
        """Pick (seq, start, n) prefill chunks for this step (`reserve` tokens of the budget are taken
        by decode rows riding along in a mixed step)."""
        chunks = []
        budget = self.max_prefill_tokens
        if reserve and self.mixed_prefill_tokens > 0:
            budget = min(budget, self.mixed_prefill_tokens + reserve)
        budget -= reserve
        # continue partially-prefilled running sequences first
        for s in self.running:
            if s.computed < len(s.prompt) and budget > 0:
                n = min(len(s.prompt) - s.computed, budget)
                chunks.append((s, s.computed, n))
                budget -= n
        with self.lock:
            while self.waiting and budget > 0 and len(self.running) < self.max_batch:
                s = self.waiting[0]
                need = len(s.prompt) + s.params.max_new_tokens
                if not self.bm.can_allocate(s.id, need):
                    break
                if s.params.uses_processors():
                    self._ensure_hist()
                    # one row per running sequence (max_batch rows, len(running) < max_batch here): none free
                    # means finished sequences' rows are still held for the in-flight step; the next collect
                    # releases them
                    if not self._hist_free:
                        break
                    s.hist_row = self._hist_free.pop()
                    self._write_bias(s)
                self.waiting.popleft()
                self.bm.ensure(s.id, need)
                s.status = RUNNING
                self.running.append(s)
                n = min(len(s.prompt), budget)
                chunks.append((s, 0, n))
                budget -= n
        return chunks

    def abort(self, s: Sequence):
        """Cancel a sequence (request timeout / client gone); applied at the next step boundary."""
        with self.lock:
            self._aborts.append(s)

    def _apply_aborts(self):
        with self.lock:
            ab, self._aborts = self._aborts, []
            for s in ab:
                if s in self.waiting:
                    self.waiting.remove(s)
                    s.status, s.finish_reason, s.t_done = FINISHED, "abort", time.perf_counter()
                    s.done.set()
        for s in ab:
            if s in self.running:
                self._finish(s, "abort")

    def _fault_hooks(self):
        f = faults.faults()
        if not f:
            return
        if "engine_crash_at_step" in f and faults.tick("engine_crash_at_step") >= int(f["engine_crash_at_step"]):
            raise faults.FaultInjected("injected engine failure")
        if "step_delay_ms" in f:
            time.sleep(float(f["step_delay_ms"]) / 1000.0)

    def step(self):
        """One engine step. Returns the sequences that finished in it (with asynchronous decode:
        whose last token was read back in it). Under TP a failed collective raises CommError."""
        fin = self._step()
        if self.comm is not None and self.tp_size > 1:
            self.comm.check()
        return fin

    def _step(self):
        self._pin_idx ^= 1
        self._pin = self._pins[self._pin_idx]
        self._pin_off = 0
        fin = []
        if self._aborts:
            fin += self._drain()
            self._apply_aborts()
        self._fault_hooks()
        n_ready = sum(1 for s in self.running if s.computed >= len(s.prompt)) if self.mixed_steps else 0
        chunks = self._admit(reserve=n_ready)
        if chunks:
            fin += self._drain()
            rows = []
            if self.mixed_steps:
                # mixed step: every running sequence past its prompt rides along as a 1-token chunk (its
                # last sampled token), so a long prefill does not stall the decoding requests
                inchunk = set(id(c[0]) for c in chunks)
                rows = [(s, s.length - 1, 1) for s in self.running
                        if id(s) not in inchunk and s.computed >= len(s.prompt) and s.computed == s.length - 1]
            return fin + self._prefill(chunks + rows, n_decode=len(rows))
        ready = [s for s in self.running if s.computed >= len(s.prompt)]
        if ready and self._needs_full_vocab(ready):
            fin += self._drain()
            ready = [s for s in self.running if s.computed >= len(s.prompt)]
            return fin + self._decode(ready, full_vocab=True)
        if ready and self.async_decode:
            return fin + self._decode_async(ready)
        fin += self._drain()
        ready = [s for s in self.running if s.computed >= len(s.prompt)]
        if ready:
            return fin + self._decode(ready)
        return fin

    def run_until_done(self, callback=None):
        finished = []
        while self.has_work():
            f = self.step()
            finished.extend(f)
            if callback:
                for s in f:
                    callback(s)
        return finished

    def generate(self, prompts, params: SamplingParams, seeds=None):
        seqs = [self.add_request(p, params, seed=None if seeds is None else seeds[i]) for i, p in enumerate(prompts)]
        self.run_until_done()
        return [s.out for s in seqs]

    # ------------------------------------------------------------------ helpers
    def _h2d_i32(self, host_list):
        """Stage a host int list / int32 array through a pinned buffer. Two buffers alternate per step
        (step() flips _pin_idx and resets the offset). Invariant: pin[i] is reused by step t+2 only;
        every path that enqueues step t+1 first synchronises step t-1 (a synchronous step ends with a
        device->host sync; the asynchronous decode pipeline _collect()s step t-1 before returning from
        step t+1, and _drain()s before any prefill), so step t-1's H2D copies out of pin[i] have
        completed before step t+1 overwrites it. A third in-flight step would break this."""
        if isinstance(host_list, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(host_list, dtype=np.int32))
        else:
            t = torch.tensor(host_list, dtype=torch.int32)
        if not self.is_cuda:
            return t
        n = t.numel()
        if self._pin_off + n > self._pin.numel():
            cap = max(1 << 20, 2 * (self._pin_off + n))
            torch.cuda.current_stream(self.device).synchronize()
            self._pin = torch.empty(cap, dtype=torch.int32, pin_memory=True)
            self._pins[self._pin_idx] = self._pin
            self._pin_off = 0
        buf = self._pin[self._pin_off:self._pin_off + n]
        self._pin_off += n
        buf.copy_(t.reshape(-1))
        return buf.to(self.device, non_blocking=True).reshape(t.shape)

    def _finish(self, s, reason, defer_free=False):
        s.status = FINISHED
        s.finish_reason = reason
        s.t_done = time.perf_counter()
        if defer_free:  # a step still in flight writes this sequence's KV row (and its history row)
            self._free_after.append(s.id)
        else:
            self.bm.free(s.id)
        if s.hist_row >= 0:
            (self._hist_after if defer_free else self._hist_free).append(s.hist_row)
            s.hist_row = -1
        self.running.remove(s)
        s.done.set()

    def _accept(self, s, tok, lp=None):
        """lp: (token logprob, alternatives) of a request with logprobs, accepted with (and only with) its token."""
        if s.t_first is None:
            s.t_first = time.perf_counter()
        s.out.append(int(tok))
        if s.logprobs is not None:
            s.logprobs.append(lp[0])
            s.top_logprobs.append(lp[1])
        p = s.params
        if not p.ignore_eos and (int(tok) in self.eos or int(tok) in p.stop_token_ids):
            return "stop"
        if len(s.out) >= p.max_new_tokens:
            return "length"
        if s.length >= self.max_model_len:
            return "length"
        return None

    def _needs_full_vocab(self, seqs):
        """True if a sampled request's top_k does not fit the K-wide candidate lists (top_k = 0 means
        "disabled" as in transformers' TopKLogitsWarper, top_k > K): such a step samples from the full
        vocabulary (exact, slower, outside the decode graph) instead of silently clamping top_k."""
        bad = any(s.params.do_sample and s.params.temperature > 0 and not (0 < s.params.top_k <= self.K)
                  for s in seqs)
        if bad and not self._warned_topk:
            log.warning("top_k outside 1..%d requested: sampling those steps from the full vocabulary", self.K)
            self._warned_topk = True
        return bad

    def _sample_full_vocab(self, logits, seqs, proc=None):
        """Exact temperature -> top-k (if 0 < top_k) -> top-p -> multinomial over the whole vocabulary
        (transformers' LogitsProcessor order, [dep] generation/utils.py:1311-1322). Under TP the vocab
        shards are all-gathered first. Uniforms come from torch.Generator(seed * 1000003 + step), as in
        the torch backend's sampler. `proc`: the logit processors' argument block (_apply_processors), applied
        first, on this rank's shard. Returns (tokens, the per-sequence logprob values in _lp_values' form of the
        rows that ask, computed from the gathered fp32 row with the reference functions; None if no row asks)."""
        w = self.model.w
        if proc is not None:
            self._apply_processors(logits[:, :w.vocab_valid] if w.vocab_valid < logits.shape[1] else logits, proc)
        lg = logits[:, :w.vocab_valid].float().contiguous()
        if self.tp_size > 1:
            import torch.distributed as dist

            # every rank contributes its FULL (padded) shard width -- the last shard is narrower when
            # vocab_size % tp != 0, and collectives need equal sizes -- with -inf in the pad columns;
            # the concatenation is then cut back to vocab_size
            lp = logits.float().clone()
            lp[:, w.vocab_valid:] = float("-inf")
            if lg.is_cuda and self.comm is not None and self.comm.ipc is None:
                parts = [torch.empty_like(lp) for _ in range(self.tp_size)]
                dist.all_gather(parts, lp.contiguous(), group=self.tp_group)
            else:  # host-side over the gloo group (CPU / peer-mapped ranks)
                grp = getattr(self.comm, "cpu_group", None) or self.tp_group
                lp = lp.cpu()
                parts = [torch.empty_like(lp) for _ in range(self.tp_size)]
                dist.all_gather(parts, lp, group=grp)
            lg = torch.cat([p.cpu() for p in parts], 1)[:, :self.model.cfg.vocab_size]
        lg = lg.cpu()
        toks = []
        for b, s in enumerate(seqs):
            p = s.params
            x = lg[b]
            if not p.do_sample or p.temperature <= 0:
                toks.append(int(torch.argmax(x)))
                continue
            x = x / p.temperature
            if p.top_k > 0:
                kth = torch.topk(x, min(p.top_k, x.numel())).values[-1]
                x = torch.where(x < kth, torch.full_like(x, float("-inf")), x)
            sv, order = torch.sort(x, descending=True)
            probs = torch.softmax(sv, 0)
            keep = (torch.cumsum(probs, 0) - probs) < p.top_p
            keep[0] = True
            q = torch.where(keep, probs, torch.zeros_like(probs))
            c = torch.cumsum(q, 0)
            g = torch.Generator().manual_seed((int(s.seed) * 1000003 + len(s.out)) & 0x7FFFFFFFFFFFFFFF)
            u = float(torch.rand(1, generator=g)) * float(c[-1])
            j = min(int(torch.searchsorted(c, torch.tensor([u]), right=True)[0]), int(keep.sum()) - 1)
            toks.append(int(order[j]))
        if not any(s.logprobs is not None for s in seqs):
            return toks, None
        from ..ops import reference as R

        vals = []
        for b, s in enumerate(seqs):
            if s.logprobs is None:
                vals.append(None)
                continue
            x = lg[b:b + 1]
            V = x.shape[1]
            sv, order = torch.sort(x, descending=True, stable=True)  # one list: the whole row, (value desc, id asc)
            _, tl, tp, ti = R.logprobs_finish(R.lse_partials(x, lse_chunks(V, 1)), sv, order.int(), V,
                                              torch.tensor([toks[b]], dtype=torch.int32),
                                              torch.tensor([s.params.logprobs], dtype=torch.int32))
            k = s.params.logprobs
            vals.append((float(tl[0]), [(int(ti[0, j]), float(tp[0, j])) for j in range(k)]))
        return toks, vals

    def _sample_rows(self, logits, v, out=None, proc=None, lp=None):
        """v: the views of the step block (its sampling section is read here).
        `proc` (optional): the logit processors' argument block; their kernel then runs in place on the
        logits before the candidate top-k (temperature / top-k / top-p follow, as in transformers).
        `lp` (optional): the logprob block (nlp [B] on the device, buf = the output words of _lp_views): two
        more launches, lse_partials next to the top-k on the same logits view and logprobs_finish after the
        sampler, on the candidates it sampled from."""
        be = self.model.be
        w = self.model.w
        lg = logits[:, :w.vocab_valid] if w.vocab_valid < logits.shape[1] else logits
        if proc is not None:
            self._apply_processors(lg, proc)
        # chunk count from the padded shard width so every TP rank gathers equal-sized lists,
        # and all ranks' candidates together fit the sampler's 2048-entry merge
        from ..ops.native import topk_chunks
        chunks = topk_chunks(logits.shape[1], self.K, min(512, 2048 // self.tp_size))
        if logits.shape[0] <= SMALL_BATCH_TOPK_MAX_B:
            # small decode batch: 7 workgroups of ~18k logits each left the top-k latency-bound (25 us
            # at batch 1); ~4k-entry chunks use ~31 CUs and the sampler merges up to 2048 candidates
            chunks = max(1, min(logits.shape[1] // SMALL_BATCH_TOPK_CHUNK, (2048 // self.tp_size) // self.K, 64))
        cv, ci = be.topk_candidates(lg.contiguous() if not lg.is_contiguous() else lg, self.K,
                                    vocab_offset=w.vocab_offset, chunks=chunks)
        part = None
        if lp is not None:
            # chunk count from the padded shard width: every TP rank contributes the same number of partials.
            # Like the top-k's above it also goes with the rows of this call (the bucket inside a graph, n on the
            # eager path): the default buckets hold 64, so both paths land on the same side of the batch-64
            # threshold and the lse bits agree; a custom `graph_buckets` that serves n <= 64 from a larger
            # bucket chunks the two paths differently, and their lse then agree to rounding only.
            part = be.lse_partials(lg, lse_chunks(logits.shape[1], logits.shape[0]))
        if self.tp_size > 1:
            cv, ci = self._gather_candidates(cv, ci)
            if part is not None:
                part = self._gather_partials(part)
        tok = be.sample_candidates(cv, ci, v["temps"], v["top_k"], v["top_p"], v["seeds"], v["steps"], list_len=self.K)
        if lp is not None:
            o_lse, o_tl, o_tp, o_ti = self._lp_views(lp["buf"], lp["n"])
            be.logprobs_finish(part, cv, ci, self.K, tok, lp["nlp"], o_lse, o_tl, o_tp, o_ti)
        if out is not None:
            out.copy_(tok)
            return out
        return tok

    def _gather_candidates(self, cv, ci):
        if self.comm is not None:
            return self.comm.gather_candidates(cv, ci)
        import torch.distributed as dist

        B, K = cv.shape
        if cv.is_cuda:
            gv = torch.empty((self.tp_size, B, K), dtype=cv.dtype, device=cv.device)
            gi = torch.empty((self.tp_size, B, K), dtype=ci.dtype, device=ci.device)
            dist.all_gather_into_tensor(gv, cv.contiguous(), group=self.tp_group)
            dist.all_gather_into_tensor(gi, ci.contiguous(), group=self.tp_group)
        else:  # gloo (CPU plumbing / tests)
            lv = [torch.empty_like(cv) for _ in range(self.tp_size)]
            li = [torch.empty_like(ci) for _ in range(self.tp_size)]
            dist.all_gather(lv, cv.contiguous(), group=self.tp_group)
            dist.all_gather(li, ci.contiguous(), group=self.tp_group)
            gv, gi = torch.stack(lv), torch.stack(li)
        return gv.permute(1, 0, 2).reshape(B, self.tp_size * K).contiguous(), \
            gi.permute(1, 0, 2).reshape(B, self.tp_size * K).contiguous()

    def _gather_partials(self, part):
        """lse partials [B, C, 2] of every TP rank -> [B, tp * C, 2], rank-major (identical on every rank)."""
        if self.comm is not None:
            return self.comm.gather_partials(part)
        import torch.distributed as dist

        B, C, _ = part.shape
        if part.is_cuda:
            g = torch.empty((self.tp_size, B, C, 2), dtype=part.dtype, device=part.device)
            dist.all_gather_into_tensor(g, part.contiguous(), group=self.tp_group)
        else:  # gloo (CPU plumbing / tests)
            lp = [torch.empty_like(part) for _ in range(self.tp_size)]
            dist.all_gather(lp, part.contiguous(), group=self.tp_group)
            g = torch.stack(lp)
        return g.permute(1, 0, 2, 3).reshape(B, self.tp_size * C, 2).contiguous()

    # ------------------------------------------------------------------ prefill
    def _prefill_input(self, chunks):
        """Packed StepInput for prefill chunks [(seq, start, n)] + the sequences whose prompt ends here.
        Built with numpy slices (a 32k-token step took ~20 ms of per-token Python before)."""
        ids, pos, slots, cu, kvl, qlens, out_rows, out_seqs = [], [], [], [0], [], [], [], []
        bts = np.zeros((len(chunks), self.max_blocks), dtype=np.int32)
        for ci, (s, start, n) in enumerate(chunks):
            table = np.asarray(self.bm.table(s.id), dtype=np.int32)
            p = np.arange(start, start + n, dtype=np.int32)
            if start + n <= len(s.prompt):
                ids.append(s.prompt_np[start:start + n])
            else:  # a decode row of a mixed step: the generated tokens past the prompt
                ids.append(np.asarray([s.token_at(i) for i in range(start, start + n)], dtype=np.int32))
            pos.append(p)
            slots.append(table[p // BLOCK] * BLOCK + p % BLOCK)
            cu.append(cu[-1] + n)
            kvl.append(start + n)
            qlens.append(n)
            nb = min(len(table), self.max_blocks)
            bts[ci, :nb] = table[:nb]
            if start + n == len(s.prompt) or (start + n == s.length and start >= len(s.prompt)):
                out_rows.append(cu[-1] - 1)
                out_seqs.append(s)
        from ..ops.native import build_last_rows_lists, build_prefill_tiles

        m = self.model
        tiles = build_prefill_tiles(qlens, m.Hq, m.Hkv)
        meta = AttnMeta("prefill", self._h2d_i32(kvl), self._h2d_i32(bts), cu_q=self._h2d_i32(cu),
                        tiles=tiles.to(self.device), host_kv_lens=kvl, host_q_lens=qlens)
        ntok = cu[-1]
        # the rows read after the last decoder layer (models/llama.py:_last_rows): with none (no prompt ends in
        # this chunk) a model that cuts its last layer gets the empty list, any other the last row as before
        cuts = getattr(m, "prefill_last_rows_enabled", None)
        cuts = self.tp_size == 1 and cuts is not None and cuts()
        m_tiles = None
        if cuts and out_rows:
            tl, mt = build_last_rows_lists(qlens, out_rows, m.Hq, m.Hkv, tiles=tiles)
            meta.tiles_last, m_tiles = self._h2d_i32(tl.numpy()), self._h2d_i32(mt.numpy())
        inp = StepInput(self._h2d_i32(np.concatenate(ids)), self._h2d_i32(np.concatenate(pos)),
                        self._h2d_i32(np.concatenate(slots)), meta,
                        self._h2d_i32(out_rows if out_rows or cuts else [ntok - 1]), m_tiles=m_tiles)
        if self._hist is not None and any(s.hist_row >= 0 for s, _, _ in chunks):
            # the step's tokens enter the history of the sequences with logit processors: one scatter launch
            # (per-token history row, -1 = skip); a chunked prompt fills its row chunk by chunk
            hrows = np.concatenate([np.full(n, s.hist_row, dtype=np.int32) for s, _, n in chunks])
            m.be.hist_write(inp.ids, self._h2d_i32(hrows), inp.positions, self._hist)
        return inp, out_seqs, ntok

    @staticmethod
    def _split_chunks(chunks, parts):
        """Cut the packed token stream into `parts` nearly equal consecutive pieces (a chunk may be
        cut in two: its second piece continues the same sequence at a later position)."""
        total = sum(n for _, _, n in chunks)
        target = -(-total // parts)
        out, cur, room = [], [], target
        for s, start, n in chunks:
            while n > 0:
                k = min(n, room)
                cur.append((s, start, k))
                start, n, room = start + k, n - k, room - k
                if room == 0 and len(out) < parts - 1:
                    out.append(cur)
                    cur, room = [], target
        if cur:
            out.append(cur)
        return out

    def _prefill(self, chunks, n_decode=0):
        t0 = time.perf_counter()
        m = self.model
        ntok = sum(n for _, _, n in chunks)
        comm = getattr(m, "comm", None)
        overlap = (self.tp_size > 1 and comm is not None and hasattr(comm, "all_reduce_async")
                   and ntok >= self.tp_overlap_min_tokens and not getattr(m, "seq_parallel", False))
        if overlap:
            groups = self._split_chunks(chunks, 2)
            built = [self._prefill_input(g) for g in groups]
            hs = m.hidden_states_microbatched([b[0] for b in built])
            out_seqs = [s for b in built for s in b[1]]
            parts = [m.logits(h) for h, b in zip(hs, built) if b[1]]
            logits = torch.cat(parts, 0) if parts else None
        else:
            inp, out_seqs, _ = self._prefill_input(chunks)
            logits = m.forward(inp) if out_seqs else None
            if logits is None:
                m.hidden_states(inp)
        finished = []
        vals = None
        if out_seqs:
            full_vocab = self._needs_full_vocab(out_seqs)
            n = len(out_seqs)
            v = self._eager_block(out_seqs, self._step_key(out_seqs, full_vocab))
            # logit processors of the sampled rows: their history (prompt, or prompt + generated for a mixed
            # step's decode rows) was completed by this step's scatter, so the kernel stores no ids
            proc = dict(v, ids=None) if "rows" in v else None
            if full_vocab:
                tok, vals = self._sample_full_vocab(logits, out_seqs, proc=proc)
            else:
                # the first generated token's logprobs: the same two launches on this eager sampling call
                lp = self._lp_block(v, n)
                tok = self._sample_rows(logits, v, proc=proc, lp=lp).cpu().tolist()
                if lp is not None:
                    vals = self._lp_values(lp["buf"].cpu(), n, out_seqs)
        else:
            tok = []
            if self.is_cuda:
                torch.cuda.current_stream(self.device).synchronize()
        for s, start, n in chunks:
            s.computed = start + n
        for i, (s, t) in enumerate(zip(out_seqs, tok)):
            r = self._accept(s, t, vals[i] if vals is not None else None)
            if r:
                self._finish(s, r)
                finished.append(s)
        self.stats["prefill_steps"] += 1
        self.stats["prefill_tokens"] += ntok - n_decode
        if n_decode:
            self.stats["mixed_decode_tokens"] = self.stats.get("mixed_decode_tokens", 0) + n_decode
        self.stats["prefill_s"] += time.perf_counter() - t0
        return finished

    # ------------------------------------------------------------------ decode
    def _bucket(self, n):
        for b in self.buckets:
            if b >= n:
                return b
        return n

    def _bt_row(self, s, need_blocks):
        """Cached, max_blocks-padded numpy block-table row of a sequence. Blocks for prompt +
        max_new_tokens are allocated at admission, so the row is built once per sequence (the
        per-step list -> array conversion was ~10 us per sequence)."""
        row = getattr(s, "_bt_np", None)
        if row is None or s._bt_nb < need_blocks:
            table = self.bm.table(s.id)
            nb = min(len(table), self.max_blocks)
            row = np.zeros(self.max_blocks, dtype=np.int32)
            row[:nb] = table[:nb]
            s._bt_np, s._bt_nb = row, nb
        return row

    def _decode_graph(self, key):
        """Decode graph of a GraphKey (bucket, processors, logprobs, penalties), captured lazily; the entries
        already captured stay the objects they are. entry["layout"] is the StepLayout of its packed buffer
        (ONE H2D copy per step), entry["views"] the named views the graph reads.
        - The plain entry is what every step of requests without opt-in features replays, and the only one
          warmup_graphs captures.
        - processors: the processor kernel between lm_head and the top-k, its per-row arguments in the block.
        - penalties (implies processors): the penalty form of that launch, four more words per row.
        - logprobs: the two logprob launches around the sampler, the rows' alternative counts (nlp) in the
          block, and entry["lp"]["buf"] as the values' device buffer."""
        if key in self.graphs:
            return self.graphs[key]
        from ..ops.native import decode_partitions

        m = self.model
        dev = self.device
        B = key.bucket
        layout = StepLayout(B, self.max_blocks, key.processors, key.penalties, key.logprobs)
        packed = torch.zeros(layout.words, dtype=torch.int32, device=dev)
        v = layout.views(packed)
        kvl, carry = v["kv_lens"], v["carry"]
        pt, mp = decode_partitions(self.max_model_len, B, m.Hkv)
        ws_o = torch.empty((B, m.Hq, mp, m.D), dtype=torch.float32, device=dev) if mp > 1 else None
        ws_ml = torch.empty((B, m.Hq, mp, 2), dtype=torch.float32, device=dev) if mp > 1 else None
        meta = AttnMeta("decode", kvl, v["block_table"], part_tiles=pt, max_parts=mp, ws_o=ws_o, ws_ml=ws_ml)
        out_tok = self._tok_out[:B]
        inp = StepInput(v["ids"], v["pos"], v["slots"], meta, None, carry=carry, carry_src=self._tok_out)
        # the processor kernel stores ids[b] (already resolved by the embedding kernel for carried rows) at
        # hist[row][pos[b]] before it reads the row's history
        proc = v if key.processors else None
        lp = self._lp_block(v, B)

        def run():
            self._sample_rows(m.forward(inp), v, out=out_tok, proc=proc, lp=lp)

        entry = dict(layout=layout, packed=packed, views=v, out=out_tok, run=run, graph=None, meta=meta, inp=inp,
                     proc=proc, lp=lp)
        if self.use_graphs:
            kvl.fill_(1)  # scratch-only rows while capturing
            carry.fill_(-1)
            if proc is not None:
                proc["rows"].fill_(-1)  # no history row is touched while capturing
            if lp is not None:
                lp["nlp"].fill_(-1)  # no logprob output is written while capturing
            # the eager warm-up runs below sample into the shared _tok_out, which may hold the in-flight
            # step's tokens that the next step carries (a graph captured lazily mid-pipeline): restore it
            saved = self._tok_out.clone()
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                for _ in range(2):
                    run()
            torch.cuda.current_stream(dev).wait_stream(s)
            # Engines are reference cycles (graphs -> entry -> run -> engine), so a dead one keeps its captured
            # graphs until the collector runs, and torch no longer collects before a capture. On ROCm a CUDAGraph's
            # destructor synchronises the device, which is illegal inside a capture and aborts the process:
            # collect now, so that no dead graph is left for a collection that starts inside the capture below.
            gc.collect()
            g = torch.cuda.CUDAGraph()
            # captured on the warm-up stream: stream-keyed native state (the persistent decode MLP's
            # arrival counters, ops/native.py _me_workspace) was allocated by the warm-up runs above
            with torch.cuda.graph(g, stream=s):
                run()
            self._tok_out.copy_(saved)
            entry["graph"] = g
        self.graphs[key] = entry
        return entry

    def warmup_graphs(self, sizes=None):
        if not self.is_cuda:  # CPU plumbing: eager decode, nothing to capture
            return
        for b in sizes or self.buckets:
            self._decode_graph(graph_key(b))
        # tensor parallel: leave warm-up together. A rank still capturing (host-bound, seconds on a loaded
        # host) would otherwise keep the others' first collectives spinning in their bounded peer waits.
        grp = getattr(self.comm, "cpu_group", None)
        if self.tp_size > 1 and grp is not None:
            import torch.distributed as dist

            torch.cuda.synchronize()
            dist.barrier(group=grp)

    # ------------------------------------------------------------------ asynchronous decode
    def _decode_async(self, ready):
        t0 = time.perf_counter()
        prev = self._inflight
        prev_row = {} if prev is None else {id(s): i for i, s in enumerate(prev["seqs"])}
        seqs = []
        for s in ready:
            if id(s) in prev_row:  # its in-flight token will be accepted: does it get another step?
                L = len(s.out) + 1
                if L >= s.params.max_new_tokens or s.length + 1 >= self.max_model_len:
                    continue
            seqs.append(s)
        if not seqs:
            return self._drain()
        n = len(seqs)
        key = self._step_key(seqs)
        e = self._decode_graph(key)
        # carried rows read their id from the previous step's sampled tokens (the shared device buffer
        # _tok_out, row = that step's row) inside the graph's embedding kernel: no extra copy / gather
        host = self._pack(e["layout"], seqs, [prev_row.get(id(s), -1) for s in seqs])
        e["packed"].copy_(self._h2d_i32(host), non_blocking=True)
        forced = self._engine_fault_hook()
        if self._timing is not None:
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea.record()
            e["graph"].replay()
            eb.record()
            self._timing.append((ea, eb))
        else:
            e["graph"].replay()
        if forced:
            self._engine_fault_hook(release=True)
        self._out_idx ^= 1
        host_out = self._out_pins[self._out_idx]
        host_out[:n].copy_(e["out"][:n], non_blocking=True)
        lp_host = None
        if key.logprobs:  # the step's logprob values ride to the host with its tokens: one more non-blocking copy
            lp_host = self._lp_pin(self._out_idx, self.LP_WORDS * key.bucket)
            lp_host.copy_(e["lp"]["buf"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        for s in seqs:
            s.computed = s.length + (1 if id(s) in prev_row else 0)
        cur = dict(seqs=seqs, out=e["out"], event=ev, host_out=host_out, n=n, lp_host=lp_host, B=key.bucket)
        fin = self._collect(prev, in_flight=set(id(s) for s in seqs))
        if fin is None:  # prev failed in-kernel; cur consumed its tokens on the device
            self._recover_engine_fault([prev, cur])
            self.stats["decode_s"] += time.perf_counter() - t0
            return []
        self._inflight = cur
        self.stats["decode_steps"] += 1
        self._count_batch(n)
        self.stats["decode_s"] += time.perf_counter() - t0
        return fin

    def _count_batch(self, n):
        """Decode steps per batch size (stats["decode_batch_hist"]): how well the schedule keeps the
        weight stream of each decode step amortised over many sequences."""
        h = self.stats.setdefault("decode_batch_hist", {})
        h[n] = h.get(n, 0) + 1

    def _collect(self, step, in_flight=frozenset()):
        """Wait for an in-flight decode step, accept its tokens, free what it no longer touches."""
        if step is None:
            return []
        step["event"].synchronize()
        self._free_deferred()  # rows of the step before `step`: done with those blocks now
        if self._kernel_fault():
            return None  # the caller discards this step (and the one in flight behind it)
        tok = step["host_out"][:step["n"]].tolist()
        # logprob values are accepted one step late with their token; a discarded row's are dropped with it
        vals = self._lp_values(step["lp_host"], step["B"], step["seqs"]) if step.get("lp_host") is not None else None
        finished = []
        for i, (s, t) in enumerate(zip(step["seqs"], tok)):
            if s.status == FINISHED:  # stopped (or aborted) before this step's token was read
                continue
            r = self._accept(s, t, vals[i] if vals is not None else None)
            self.stats["decode_tokens"] += 1
            if r:
                self._finish(s, r, defer_free=id(s) in in_flight)
                finished.append(s)
        return finished

    def _kernel_fault(self) -> int:
        """Error code a bounded in-kernel wait reported during the steps synchronised so far (the persistent
        decode MLP's hand-off, ops/native.py mlp_engine_fault): host-mapped words, read after the step's
        event sync at no extra cost. 0 = healthy."""
        if not self.is_cuda:
            return 0
        from ..ops import native
        return native.mlp_engine_fault(self.device)

    def _engine_fault_hook(self, release=False):
        """RAGK_FAULTS=mlp_engine_timeout_at_step=N: the N-th decode step's persistent MLP launches get a
        one-tick deadline (every wait gives up) -- the recovery path's test."""
        from ..ops import native
        if release:
            native.mlp_engine_force_timeout(0, self.device)
            return False
        at = faults.value("mlp_engine_timeout_at_step")
        if at is None or not self.is_cuda or faults.tick("mlp_engine_timeout_at_step") != int(at):
            return False
        native.mlp_engine_force_timeout(1, self.device)
        return True

    def _recover_engine_fault(self, steps):
        """A persistent decode MLP launch gave up a wait: its step's rows (and those of the step in flight
        behind it, which consumed its tokens) are garbage and are NOT accepted. Wait for the device, re-arm
        the counters, turn the engine off for this process (its graphs are recaptured on the separate
        kernels on demand) and rewind every affected sequence to its last accepted token, so the next decode
        step recomputes those rows; the KV rows they wrote are rewritten by the recomputation."""
        code = self._kernel_fault()
        if self.is_cuda:
            from ..ops import native
            torch.cuda.synchronize(self.device)
            native.mlp_engine_rearm(self.device)
            native.MLP_ENGINE = False
        self.graphs.clear()
        self._inflight = None
        self._free_deferred()
        n = 0
        for step in steps:
            if step is None:
                continue
            for s in step["seqs"]:
                if s.status != FINISHED:
                    s.computed = s.length - 1
                    n += 1
        self.stats["engine_faults"] = self.stats.get("engine_faults", 0) + 1
        log.error("persistent decode MLP: a wait gave up (code %d); %d rows of the last decode steps discarded "
                  "and recomputed on the separate kernels (engine off for this process)", code, n)

    def _drain(self):
        """Complete the in-flight decode step (before a prefill, an abort, or when nothing is left)."""
        if self._inflight is None:
            return []
        t0 = time.perf_counter()
        step, self._inflight = self._inflight, None
        fin = self._collect(step)
        if fin is None:
            self._recover_engine_fault([step])
            self.stats["decode_s"] += time.perf_counter() - t0
            return []
        self._free_deferred()
        self.stats["decode_s"] += time.perf_counter() - t0
        return fin

    def _decode(self, seqs, full_vocab=False):
        t0 = time.perf_counter()
        n = len(seqs)
        finished = []
        if not seqs:
            return finished
        key = self._step_key(seqs, full_vocab)
        vals = None
        if self.is_cuda:
            e = self._decode_graph(key)
            e["packed"].copy_(self._h2d_i32(self._pack(e["layout"], seqs)), non_blocking=True)
            if full_vocab:  # eager forward, exact sampler over the whole vocabulary
                proc = {k: t[:n] for k, t in e["proc"].items()} if key.processors else None
                tok, vals = self._sample_full_vocab(self.model.forward(e["inp"])[:n], seqs, proc=proc)
            else:
                forced = self._engine_fault_hook()
                if e["graph"] is not None:
                    e["graph"].replay()
                else:
                    e["run"]()
                if forced:
                    self._engine_fault_hook(release=True)
                tok = e["out"][:n].cpu().tolist()
                if key.logprobs:
                    vals = self._lp_values(e["lp"]["buf"].cpu(), key.bucket, seqs)
            if self._kernel_fault():  # synchronised by the token read-back above
                self._recover_engine_fault([dict(seqs=seqs)])
                self.stats["decode_s"] += time.perf_counter() - t0
                return finished
        else:
            v = self._eager_block(seqs, key, self.max_blocks)
            meta = AttnMeta("decode", v["kv_lens"], v["block_table"], host_kv_lens=v["kv_lens"].tolist())
            logits = self.model.forward(StepInput(v["ids"], v["pos"], v["slots"], meta, None))
            proc = v if key.processors else None
            if full_vocab:
                tok, vals = self._sample_full_vocab(logits, seqs, proc=proc)
            else:
                lp = self._lp_block(v, n)
                tok = self._sample_rows(logits, v, proc=proc, lp=lp).tolist()
                if lp is not None:
                    vals = self._lp_values(lp["buf"], n, seqs)
            if self._kernel_fault():
                self._recover_engine_fault([dict(seqs=seqs)])
                self.stats["decode_s"] += time.perf_counter() - t0
                return finished
        for s in seqs:
            s.computed = s.length
        for i, (s, t) in enumerate(zip(seqs, tok)):
            r = self._accept(s, t, vals[i] if vals is not None else None)
            if r:
                self._finish(s, r)
                finished.append(s)
        self.stats["decode_steps"] += 1
        self._count_batch(n)
        self.stats["decode_tokens"] += n
        self.stats["decode_s"] += time.perf_counter() - t0
        return finished
