"""Flask REST API -- drop-in surface of the reference (/root/reference/llm/rag.py:122-204).

Routes (exact request/response/error contract):
  POST /generate     {"prompt": str} -> 200 {"generated_text", "context"}
                                      | 200 {"generated_text": "No relevant information found in the index."}
                                      | 500 {"error": str}
  POST /query        alias of /generate (BASELINE.json names a "/query" API)
  POST /upload_pdf   multipart "file" -> 200 {"message": "PDF processed and indexed successfully. N chunks created."}
                                       | 400 {"error": "No file part" | "No selected file" | "Invalid file format"}
  GET  /index_info   -> {"total_vectors", "dimension", "total_chunks", "sample_chunks"} | 500 {"error"}
New: GET /healthz (liveness), GET /readyz (weights + index loaded), GET /metrics (Prometheus).
New (documents can be listed, removed, replaced and filtered on; the reference can only add):
  POST /generate     optional "filenames": [str, ...] -> the context comes from these documents only
  POST /generate     optional "rerank": false -> skip the cross-encoder stage for this query (RERANK_MODEL set);
                     "rerank": true without RERANK_MODEL -> 500 {"error"} naming it
  POST /generate     optional "repetition_penalty": float > 0, "no_repeat_ngram_size": 0..8, "min_new_tokens":
                     0..MAX_NEW_TOKENS -> override REPETITION_PENALTY / NO_REPEAT_NGRAM_SIZE / MIN_NEW_TOKENS for
                     this request (transformers' generate() semantics); a refused value -> 400 {"error"}
  POST /generate     optional "presence_penalty", "frequency_penalty": numbers in -2..2 (OpenAI's semantics: every
                     token GENERATED so far loses frequency * its count + presence; prompt tokens do not count),
                     "logit_bias": {"<token id>": number in -100..100, ...} (at most 300 entries, added to those
                     tokens' logits before everything else) -> override PRESENCE_PENALTY / FREQUENCY_PENALTY /
                     LOGIT_BIAS for this request; a refused value or a non-integer key -> 400 {"error"}
  POST /generate     optional "logprobs": N (integer 0..20; overrides LOGPROBS) -> the response gains "logprobs":
                     {"token_ids", "tokens", "token_logprobs", "top_logprobs": [[{"id", "token", "logprob"}, ...],
                     ...], "mean_logprob"} over every generated token (a final eos included): log_softmax of the
                     fp32 logits after the logit processors, before temperature / top-k / top-p, with the N most
                     likely alternatives per position; a bool, float, negative or > 20 value -> 400 {"error"}.
                     Without the field (and without LOGPROBS) the response keys are unchanged
  POST /generate     optional "hybrid": true | false -> fuse (or not) the BM25 lexical list with the dense one for this
                     query (HYBRID_SEARCH=rrf sets the default); "hybrid": true on a server without a lexical index,
                     or a value that is no boolean -> 400 {"error"}. With "debug" the response's "retrieved" rows
                     gain "dense_rank", "lexical_rank" (1-based, null = not in that list) and "lexical_score"
  POST /upload_pdf?replace=1 (or form field replace=1) -> the document's old chunks are replaced
  GET  /documents    -> {"documents": [{"filename", "chunks"}]}
  DELETE /documents/<filename> -> 200 {"message", "chunks_removed"} | 404 {"error"}
                                | 501 {"error"} on a row-sharded index (INDEX_SHARDED)
"""
from __future__ import annotations

import logging

from flask import Flask, Response, jsonify, request

from ..utils import metrics

log = logging.getLogger(__name__)


def create_app(service) -> Flask:
    app = Flask("rag_llm_k8s_amd")

    def _generate():
        try:
            data = request.json
            user_prompt = data.get("prompt", "")
            debug = bool(data.get("debug", False))
            filenames = data.get("filenames")
            kw = {"filenames": filenames} if filenames else {}
            if data.get("rerank") is not None:  # per-request switch of the cross-encoder stage
                kw["rerank"] = bool(data["rerank"])
            if data.get("hybrid") is not None:  # per-request switch of the BM25 + dense fusion
                if not isinstance(data["hybrid"], bool):
                    metrics.inc("requests", route="generate", status="400")
                    return jsonify({"error": '"hybrid" must be true or false (got %r)' % (data["hybrid"],)}), 400
                try:
                    kw["hybrid"] = service._hybrid_flag(data["hybrid"])
                except ValueError as e:  # no lexical index on this server
                    metrics.inc("requests", route="generate", status="400")
                    return jsonify({"error": str(e)}), 400
            # per-request logit processors: the service's default SamplingParams with these fields replaced
            over = {k: data[k] for k in service.REQUEST_PARAM_FIELDS if data.get(k) is not None}
            if over:
                try:
                    kw["params"] = service.request_params(over)
                except ValueError as e:  # a value the engine refuses
                    metrics.inc("requests", route="generate", status="400")
                    return jsonify({"error": str(e)}), 400
            out = service.generate(user_prompt, debug=debug, **kw)
            metrics.inc("requests", route="generate", status="200")
            return jsonify(out)
        except Exception as e:
            log.error("Error in generate_text: %s", str(e), exc_info=True)
            metrics.inc("requests", route="generate", status="500")
            return jsonify({"error": str(e)}), 500

    app.add_url_rule("/generate", "generate", _generate, methods=["POST"])
    app.add_url_rule("/query", "query", _generate, methods=["POST"])

    @app.route("/upload_pdf", methods=["POST"])
    def upload_pdf():
        if "file" not in request.files:
            return jsonify({"error": "No file part"}), 400
        file = request.files["file"]
        if file.filename == "":
            return jsonify({"error": "No selected file"}), 400
        if file and file.filename.endswith(".pdf"):
            if str(request.args.get("replace", request.form.get("replace", ""))).lower() in ("1", "true", "yes"):
                try:
                    n = service.ingest_pdf_bytes(file.filename, file.read(), replace=True)
                except ValueError as e:  # row-sharded index
                    return jsonify({"error": str(e)}), 501
            else:
                n = service.ingest_pdf_bytes(file.filename, file.read())
            metrics.inc("requests", route="upload_pdf", status="200")
            return jsonify({"message": f"PDF processed and indexed successfully. {n} chunks created."}), 200
        return jsonify({"error": "Invalid file format"}), 400

    @app.route("/index_info", methods=["GET"])
    def index_info():
        try:
            return jsonify(service.index_info())
        except Exception as e:
            log.error("Error in index_info: %s", str(e), exc_info=True)
            return jsonify({"error": str(e)}), 500

    @app.route("/documents", methods=["GET"])
    def documents():
        try:
            return jsonify({"documents": service.documents()})
        except Exception as e:
            log.error("Error in documents: %s", str(e), exc_info=True)
            return jsonify({"error": str(e)}), 500

    @app.route("/documents/<path:filename>", methods=["DELETE"])
    def delete_document(filename):
        try:
            n = service.delete_document(filename)
        except ValueError as e:  # row-sharded index: not supported
            metrics.inc("requests", route="delete_document", status="501")
            return jsonify({"error": str(e)}), 501
        except Exception as e:
            log.error("Error in delete_document: %s", str(e), exc_info=True)
            metrics.inc("requests", route="delete_document", status="500")
            return jsonify({"error": str(e)}), 500
        if n == 0:
            metrics.inc("requests", route="delete_document", status="404")
            return jsonify({"error": f"Document not found: {filename}"}), 404
        metrics.inc("requests", route="delete_document", status="200")
        return jsonify({"message": f"Document deleted. {n} chunks removed.", "chunks_removed": n}), 200

    @app.route("/healthz", methods=["GET"])
    def healthz():
        h = service.health()
        return jsonify(h), (200 if h["engine_alive"] else 503)

    @app.route("/readyz", methods=["GET"])
    def readyz():
        h = service.health()
        ok = h["engine_alive"] and h["ready"]
        return jsonify(h), (200 if ok else 503)

    @app.route("/metrics", methods=["GET"])
    def prom_metrics():
        body, ctype = metrics.exposition()
        return Response(body, mimetype=ctype.split(";")[0] if ctype else "text/plain")

    return app
