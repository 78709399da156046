#include "words.hpp"

#include <cstring>

namespace humid_host {

static inline int code_of(char c) {
  switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: return -1;
  }
}

bool valid_umi(std::string_view umi) {
  if (umi.empty()) return false;
  for (char c : umi)
    if (code_of(c) < 0) return false;
  return true;
}

std::string_view last_field(std::string_view s, char sep) {
  size_t p = s.rfind(sep);
  if (p == std::string_view::npos) return std::string_view();
  return s.substr(p + 1);
}

std::string_view header_umi(std::string_view header) {
  std::string_view id = header.substr(0, header.find(' '));
  std::string_view u = last_field(id, '_');
  if (valid_umi(u)) return u;
  u = last_field(id, ':');
  if (valid_umi(u)) return u;
  return std::string_view();
}

std::vector<size_t> nt_from_file(size_t files, size_t length) {
  std::vector<size_t> v(files, files ? length / files : 0);
  if (files) v.back() += length % files;
  return v;
}

WordPlan make_plan(size_t first_header_umi, size_t n_files, size_t word_nt) {
  WordPlan p;
  p.word_nt = word_nt;
  size_t from_files = word_nt > first_header_umi ? word_nt - first_header_umi : 0;
  p.take = nt_from_file(n_files, from_files);
  p.header_umi = first_header_umi < word_nt ? first_header_umi : word_nt;
  return p;
}

bool make_pattern_plan(const std::string &pattern, size_t n_files, size_t word_nt, WordPlan &plan, size_t &n_barcode,
                       std::string &err) {
  std::vector<WordPlan::Range> bc, umi;
  size_t n_c = 0, n_n = 0;
  for (size_t i = 0; i < pattern.size(); i++) {
    const char ch = pattern[i];
    if (ch != 'C' && ch != 'N' && ch != 'X') { err = "--word-pattern takes the letters C (barcode), N (UMI) and X (skipped)"; return false; }
    if (ch == 'X') continue;
    std::vector<WordPlan::Range> &to = ch == 'C' ? bc : umi;
    (ch == 'C' ? n_c : n_n)++;
    if (!to.empty() && to.back().off + to.back().len == i) to.back().len++;
    else to.push_back({i, 1});
  }
  if (pattern.empty()) { err = "--word-pattern takes a pattern of one letter or more"; return false; }
  if (n_c + n_n > word_nt || (n_files == 1 && n_c + n_n != word_nt)) {
    err = "--word-pattern: the pattern's " + std::to_string(n_c) + " C and " + std::to_string(n_n) + " N letters " +
          (n_files == 1 ? "must add up to" : "exceed") + " the word length (-n " + std::to_string(word_nt) + ")";
    return false;
  }
  plan = WordPlan();
  plan.word_nt = word_nt;
  plan.header_umi = 0;
  plan.take = nt_from_file(n_files - 1, word_nt - n_c - n_n);
  plan.take.insert(plan.take.begin(), n_c + n_n);
  plan.patterned = true;
  plan.first = bc;
  plan.first.insert(plan.first.end(), umi.begin(), umi.end());
  n_barcode = n_c;
  return true;
}

// the letters of range r that the read has (the rest is padding)
static inline std::string_view cut(std::string_view s, const WordPlan::Range &r) {
  return r.off < s.size() ? s.substr(r.off, r.len) : std::string_view();
}

// appends `want` symbols of `s` (cut or padded with a non-ACGT symbol) to the packed word
template <class Acc>
static inline void push_symbols(std::string_view s, size_t want, Acc &w, bool &filtered) {
  size_t have = s.size() < want ? s.size() : want;
  for (size_t i = 0; i < have; i++) {
    int c = code_of(s[i]);
    if (c < 0) { c = 2; filtered = true; }       // unknown base: code of 'G', word filtered
    w = (w << 2) | (Acc)c;
  }
  for (size_t i = have; i < want; i++) {         // 'N' padding of a short UMI / read
    w = (w << 2) | 2u;
    filtered = true;
  }
}

bool make_word(std::string_view first_header, const std::string_view *seqs, size_t n_files,
               const WordPlan &plan, uint64_t &word) {
  uint64_t w = 0;
  bool filtered = false;
  if (plan.header_umi > 0) push_symbols(header_umi(first_header), plan.header_umi, w, filtered);
  for (size_t f = 0; f < n_files; f++) {
    if (f == 0 && plan.patterned)
      for (const WordPlan::Range &r : plan.first) push_symbols(cut(seqs[0], r), r.len, w, filtered);
    else push_symbols(seqs[f], plan.take[f], w, filtered);
  }
  word = w;
  return filtered;
}

static inline uint8_t *copy_padded(std::string_view s, size_t want, uint8_t *out) {
  const size_t have = s.size() < want ? s.size() : want;
  memcpy(out, s.data(), have);
  if (have < want) memset(out + have, 'N', want - have);
  return out + want;
}

void gather_bases(std::string_view first_header, const std::string_view *seqs, size_t n_files,
                  const WordPlan &plan, uint8_t *out) {
  if (plan.header_umi > 0) out = copy_padded(header_umi(first_header), plan.header_umi, out);
  for (size_t f = 0; f < n_files; f++) {
    if (f == 0 && plan.patterned)
      for (const WordPlan::Range &r : plan.first) out = copy_padded(cut(seqs[0], r), r.len, out);
    else out = copy_padded(seqs[f], plan.take[f], out);
  }
}

bool make_word_wide(std::string_view first_header, const std::string_view *seqs, size_t n_files,
                    const WordPlan &plan, uint64_t word[2]) {
  unsigned __int128 w = 0;
  bool filtered = false;
  if (plan.header_umi > 0) push_symbols(header_umi(first_header), plan.header_umi, w, filtered);
  for (size_t f = 0; f < n_files; f++) {
    if (f == 0 && plan.patterned)
      for (const WordPlan::Range &r : plan.first) push_symbols(cut(seqs[0], r), r.len, w, filtered);
    else push_symbols(seqs[f], plan.take[f], w, filtered);
  }
  word[0] = (uint64_t)(w >> 64);     // the first word_nt - 32 symbols
  word[1] = (uint64_t)w;             // the last 32
  return filtered;
}

// --long-words: the symbols arrive in order, so each goes to the low end of its uint64 -- [0] takes the first
// word_nt - 32 (k - 1), every following one the next 32
struct LongAcc {
  uint64_t *out;
  size_t head_nt, p;
  void push(unsigned c) {
    const size_t col = p < head_nt ? 0 : 1 + (p - head_nt) / 32;
    out[col] = (out[col] << 2) | c;
    p++;
  }
};
static inline void push_symbols(std::string_view s, size_t want, LongAcc &w, bool &filtered) {
  const size_t have = s.size() < want ? s.size() : want;
  for (size_t i = 0; i < have; i++) {
    int c = code_of(s[i]);
    if (c < 0) { c = 2; filtered = true; }
    w.push((unsigned)c);
  }
  for (size_t i = have; i < want; i++) { w.push(2u); filtered = true; }
}

bool make_word_long(std::string_view first_header, const std::string_view *seqs, size_t n_files, const WordPlan &plan,
                    uint64_t *word) {
  const size_t k = (plan.word_nt + 31) / 32;
  memset(word, 0, k * sizeof(uint64_t));
  LongAcc w{word, plan.word_nt - 32 * (k - 1), 0};
  bool filtered = false;
  if (plan.header_umi > 0) push_symbols(header_umi(first_header), plan.header_umi, w, filtered);
  for (size_t f = 0; f < n_files; f++) push_symbols(seqs[f], plan.take[f], w, filtered);
  return filtered;
}

bool make_word_long(const std::vector<FastqRecord> &recs, const WordPlan &plan, uint64_t *word) {
  std::string_view seqs[64];
  const size_t n = recs.size() < 64 ? recs.size() : 64;
  for (size_t f = 0; f < n; f++) seqs[f] = recs[f].seq;
  return make_word_long(recs.front().name, seqs, n, plan, word);
}

bool make_word_wide(const std::vector<FastqRecord> &recs, const WordPlan &plan, uint64_t word[2]) {
  std::string_view seqs[64];
  const size_t n = recs.size() < 64 ? recs.size() : 64;
  for (size_t f = 0; f < n; f++) seqs[f] = recs[f].seq;
  return make_word_wide(recs.front().name, seqs, n, plan, word);
}

bool make_word(const std::vector<FastqRecord> &recs, const WordPlan &plan, uint64_t &word) {
  std::string_view seqs[64];
  const size_t n = recs.size() < 64 ? recs.size() : 64;
  for (size_t f = 0; f < n; f++) seqs[f] = recs[f].seq;
  return make_word(recs.front().name, seqs, n, plan, word);
}

std::string make_file_name(const std::string &path, const std::string &dir, const std::string &suffix) {
  size_t slash = path.find_last_of('/');
  std::string base = slash == std::string::npos ? path : path.substr(slash + 1);
  size_t dot = base.find('.');
  std::string out = dir + '/';
  if (dot == std::string::npos) return out + base + '_' + suffix;   // the reference throws here
  return out + base.substr(0, dot) + '_' + suffix + base.substr(dot);
}

}  // namespace humid_host
