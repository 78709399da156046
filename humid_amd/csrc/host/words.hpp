// words.hpp -- word extraction of the `humid` host: FastQ records -> 2-bit packed word + filtered.
//
// Behaviour follows /root/reference/src/fastq.cc (extractUMI_ :72-93, getNucleotides :116-144,
// makeWord :146-161, ntFromFile :220-230, makeFileName :174-181) and src/humid.cc preCompute
// :38-59; the implementation packs straight into the C-ABI word (include/humid_hip.h) instead of
// building vector<uint8_t> words.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "fastq_io.hpp"

namespace humid_host {

// UMI in a header line: text before the first space; last '_' field if it is all ACGT, else last
// ':' field if it is all ACGT, else none.  `header` may include the leading '@'.
std::string_view header_umi(std::string_view header);

bool valid_umi(std::string_view umi);                                   // non-empty, only ACGT
std::string_view last_field(std::string_view s, char sep);             // "" when sep is absent
std::vector<size_t> nt_from_file(size_t files, size_t length);         // remainder to the LAST file

struct WordPlan {
  size_t word_nt = 24;
  size_t header_umi = 0;           // symbols taken from the first file's header UMI
  std::vector<size_t> take;        // symbols taken from each file's read
  // --word-pattern: the first file's read contributes these letters instead of its first take[0] ones, range after
  // range: the barcode's (the pattern's C) in read order, then the UMI's (its N); take[0] is their total
  struct Range { size_t off, len; };
  bool patterned = false;
  std::vector<Range> first;
};
// first_header_umi: UMI length found in the first record of the first file (peekUMI)
WordPlan make_plan(size_t first_header_umi, size_t n_files, size_t word_nt);

// --word-pattern P (letters C, N, X as in UMI-tools' --bc-pattern, applied to the first file's read): the C letters in
// order are the barcode and start the word, the N letters follow, X letters are skipped; the remaining
// word_nt - #C - #N symbols come from the other files (nt_from_file over them).  No header UMI.  n_barcode = #C.
// false + a one-line message in err when the pattern cannot serve.
bool make_pattern_plan(const std::string &pattern, size_t n_files, size_t word_nt, WordPlan &plan, size_t &n_barcode,
                       std::string &err);

// One record set -> packed word (first symbol most significant).  Returns true when the word is
// filtered (a symbol outside ACGT, including 'N' padding of short UMIs/reads; coded as 'G').
// Requires plan.word_nt <= 32.
bool make_word(const std::vector<FastqRecord> &recs, const WordPlan &plan, uint64_t &word);
// the same on views (fast path: records read straight from the file mapping)
bool make_word(std::string_view first_header, const std::string_view *seqs, size_t n_files,
               const WordPlan &plan, uint64_t &word);

// 33 <= plan.word_nt <= 64: two uint64, [0] = the first word_nt-32 symbols, [1] = the last 32
bool make_word_wide(const std::vector<FastqRecord> &recs, const WordPlan &plan, uint64_t word[2]);
bool make_word_wide(std::string_view first_header, const std::string_view *seqs, size_t n_files,
                    const WordPlan &plan, uint64_t word[2]);

// --long-words, 1 <= plan.word_nt <= 512 (no --word-pattern): k = ceil(word_nt / 32) uint64, [0] = the first
// word_nt - 32 (k - 1) symbols right-aligned, every following one the next 32 (humid_dedup_run_long); up to 64 symbols
// that is what make_word / make_word_wide write
bool make_word_long(const std::vector<FastqRecord> &recs, const WordPlan &plan, uint64_t *word);
bool make_word_long(std::string_view first_header, const std::string_view *seqs, size_t n_files, const WordPlan &plan,
                    uint64_t *word);

// -P (strand-symmetric words, include/humid_hip.h): the word A.B of word_nt = 2 h nucleotides becomes the smaller of
// itself and its mirror B.A, in place (wpr uint64 per word: 1 up to 32 nucleotides, 2 beyond).  Returns true when the
// mirror was the smaller one (a bottom-strand read).
inline bool canonical_word(uint64_t *w, size_t wpr, size_t word_nt) {
  const unsigned n = (unsigned)word_nt;
  const unsigned __int128 v = wpr == 2 ? ((unsigned __int128)w[0] << 64) | w[1] : (unsigned __int128)w[0];
  const unsigned __int128 m = ((v & ((((unsigned __int128)1) << n) - 1)) << n) | (v >> n);
  if (!(m < v)) return false;
  if (wpr == 2) { w[0] = (uint64_t)(m >> 64); w[1] = (uint64_t)m; }
  else w[0] = (uint64_t)m;
  return true;
}

// getNucleotides (src/fastq.cc:116-144) as raw bytes, for the device-side packing of
// humid_dedup_run_bases: out[plan.word_nt] = the header UMI cut or padded with 'N' to plan.header_umi
// symbols, then the first plan.take[f] bytes of every file's read (the first file's ranges with --word-pattern), 'N'
// where a read is short.  The
// bytes are copied as they stand in the FastQ; the device maps and validates them.
void gather_bases(std::string_view first_header, const std::string_view *seqs, size_t n_files,
                  const WordPlan &plan, uint8_t *out);

// <dir>/<basename with _suffix inserted before the first '.'>
std::string make_file_name(const std::string &path, const std::string &dir, const std::string &suffix);

}  // namespace humid_host
