// Lexical analyzer of the BM25 index (index/lexical.py holds the pure-Python twin with the same output).
// One fixed function over the UTF-8 bytes of a text, no language knowledge:
//   token   = maximal run of bytes that are ASCII letters, ASCII digits or >= 0x80; ASCII upper case lowered
//   term id = 32-bit FNV-1a of the token's bytes, 0xFFFFFFFF remapped to 0xFFFFFFFE (the former pads tables)
// Per document: the distinct term ids ascending, their counts saturating at 65535, and the token count.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace ragk_rt {

constexpr uint32_t LEX_PAD = 0xFFFFFFFFu;

inline uint32_t lex_remap(uint32_t h) { return h == LEX_PAD ? 0xFFFFFFFEu : h; }

inline bool lex_token_byte(unsigned char c) {
  return c >= 0x80 || (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
}

// term id of every token of `text`, in order of appearance
inline void lex_tokens(const std::string& text, std::vector<uint32_t>& out) {
  out.clear();
  const size_t n = text.size();
  size_t i = 0;
  while (i < n) {
    while (i < n && !lex_token_byte((unsigned char)text[i])) ++i;
    if (i >= n) break;
    uint32_t h = 2166136261u;
    for (; i < n && lex_token_byte((unsigned char)text[i]); ++i) {
      unsigned char c = (unsigned char)text[i];
      if (c >= 'A' && c <= 'Z') c = (unsigned char)(c + 32);
      h = (h ^ c) * 16777619u;
    }
    out.push_back(lex_remap(h));
  }
}

struct LexCsr {
  std::vector<int64_t> row_ptr;  // [n + 1]
  std::vector<uint32_t> terms;   // distinct term ids of each document, ascending
  std::vector<uint16_t> tf;      // their counts, saturating
  std::vector<int32_t> doc_len;  // tokens per document
};

inline LexCsr lex_analyze_batch(const std::vector<std::string>& texts) {
  LexCsr r;
  r.row_ptr.reserve(texts.size() + 1);
  r.row_ptr.push_back(0);
  r.doc_len.reserve(texts.size());
  std::vector<uint32_t> toks;
  for (const std::string& t : texts) {
    lex_tokens(t, toks);
    r.doc_len.push_back((int32_t)std::min<size_t>(toks.size(), 0x7fffffff));
    std::sort(toks.begin(), toks.end());
    for (size_t i = 0; i < toks.size();) {
      size_t j = i;
      while (j < toks.size() && toks[j] == toks[i]) ++j;
      r.terms.push_back(toks[i]);
      r.tf.push_back((uint16_t)std::min<size_t>(j - i, 65535));
      i = j;
    }
    r.row_ptr.push_back((int64_t)r.terms.size());
  }
  return r;
}

}  // namespace ragk_rt
