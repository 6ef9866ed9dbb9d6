"""Streamlit chat UI (reference web/app.py contract: POST {LLM_SERVICE_URL}/generate {"prompt"} ->
{"generated_text"}). Unchanged request/response contract; adds a request timeout, an optional
view of the retrieved context, and a sidebar over the document routes (GET /documents, DELETE
/documents/<filename>) with a multiselect that restricts retrieval ("filenames" in the request; left
empty, the request is the reference's {"prompt"})."""
import os
from urllib.parse import quote

import requests
import streamlit as st

LLM_SERVICE_URL = os.getenv("LLM_SERVICE_URL", "http://llm-service:80")
TIMEOUT_S = float(os.getenv("LLM_TIMEOUT_S", "300"))


def list_documents():
    try:
        r = requests.get(f"{LLM_SERVICE_URL}/documents", timeout=TIMEOUT_S)
        return r.json().get("documents", []) if r.status_code == 200 else []
    except (requests.RequestException, ValueError):
        return []


docs = list_documents()
with st.sidebar:
    st.header("Documents")
    if not docs:
        st.caption("No documents indexed.")
    for doc in docs:
        name_col, del_col = st.columns([4, 1])
        name_col.write(f"{doc['filename']} ({doc['chunks']} chunks)")
        if del_col.button("Delete", key="del-" + doc["filename"]):
            try:
                r = requests.delete(f"{LLM_SERVICE_URL}/documents/{quote(doc['filename'])}", timeout=TIMEOUT_S)
            except requests.RequestException as e:
                st.error(f"Request failed: {e}")
            else:
                if r.status_code == 200:
                    st.success(r.json().get("message", "Deleted."))
                    st.rerun()
                else:
                    st.error(f"Error: {r.status_code}, {r.text}")
    only = st.multiselect("Answer from these documents only:", [doc["filename"] for doc in docs])

st.title("RAG-Enhanced LLM Chat Interface")
prompt = st.text_input("Enter your prompt:", "")
show_ctx = st.checkbox("Show retrieved context", value=False)

if st.button("Generate"):
    if not prompt:
        st.warning("Please enter a prompt.")
    else:
        body = {"prompt": prompt}
        if only:
            body["filenames"] = only
        try:
            r = requests.post(f"{LLM_SERVICE_URL}/generate", json=body, timeout=TIMEOUT_S)
        except requests.RequestException as e:
            st.error(f"Request failed: {e}")
        else:
            if r.status_code == 200:
                body = r.json()
                st.write("Generated response:")
                st.write(body["generated_text"])
                if show_ctx and body.get("context"):
                    with st.expander("Context"):
                        st.text(body["context"])
            else:
                st.error(f"Error: {r.status_code}, {r.text}")

st.write("This interface uses the Meta-Llama-3.1-8B-Instruct model served on AMD Instinct MI355X.")
