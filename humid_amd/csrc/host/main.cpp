// humid -- command-line host of the MI355X-native HUMID hot path.
//
// Keeps the reference's CLI and FastQ-in / FastQ-out contract
// (/root/reference/src/humid.cc:369-429): same flags, same log lines, same output names
// (<name>_dedup.<ext>, <name>_annotated.<ext>), same .dat statistics.  FastQ is streamed twice:
// pass 1 builds the packed words, libhumid_hip.so (include/humid_hip.h) does counts ->
// neighbours -> clusters on the GPU, pass 2 writes with the per-read (cluster_id, keep) arrays
// instead of trie.find() (src/humid.cc:223-231,276-277).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>

#include <unistd.h>

#include <atomic>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <functional>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/humid_hip.h"
#include "fastq_io.hpp"
#include "fastq_mmap.hpp"
#include <iterator>
#include <memory>
#include <thread>

#include "fast_inflate.hpp"
#include "position.hpp"
#include "sharded.hpp"
#include "words.hpp"

using namespace humid_host;

namespace {

struct Args {
  size_t word_length = 24;     // -n
  size_t distance = 1;         // -m
  std::string log_name = "/dev/stderr";   // -l
  std::string dir_name = ".";  // -d
  bool stats = false;          // -s
  bool filter = true;          // -q flips
  bool annotate = false;       // -a
  bool edit = false;           // -e
  bool maximum = false;        // -x
  std::vector<std::string> files;
  std::string dump_words;      // --dump-words (development: stop after pass 1, no GPU)
  unsigned gpus = 1;           // -g (not in the reference): ranks the read set is sharded over, one GPU each
  bool keyed = false;          // -b given (not in the reference): the first `barcode` nucleotides of the word are matched exactly
  size_t barcode = 0;          // -b
  std::vector<std::string> whitelists;   // -w (not in the reference): file of known barcodes the -b barcodes are corrected against; given several times: one file per segment of the barcode, in order
  bool max_inexact_given = false;     // --barcode-max-inexact (several -w): segments of a read's barcode that may be other than exact
  unsigned long long max_inexact = 0;
  std::string word_pattern;    // --word-pattern (not in the reference): which letters of the first file's read make the word (C barcode, N UMI, X skipped)
  bool posterior = false;      // --barcode-posterior (needs -w): barcodes with several listed neighbours are decided by base quality and abundance
  unsigned long long min_odds = 39;   // --barcode-min-odds
  int cells_mode = -1;         // --cells-top / --cells-expected / --cells-min-reads (not in the reference): HUMID_CELLS_*, the whitelist comes from the data
  unsigned cells_modes_given = 0;     // how many of the three were given
  unsigned long long cells_param = 0; // the mode's N
  bool cells_ratio_given = false;     // --cells-merge-ratio was given
  unsigned long long cells_ratio = 0; // --cells-merge-ratio (0: selected barcodes one substitution apart all stay)
  std::string dump_bc_quals;   // --dump-barcode-quals (development: the barcode qualities of pass 1, then stop, no GPU)
  bool best = false;           // -Q (not in the reference): every cluster keeps its record with the best base qualities
  std::string dump_scores;     // --dump-scores (development: the -Q scores of pass 1, then stop, no GPU)
  bool consensus = false;      // -C (not in the reference): every kept record carries the consensus of its cluster's reads
  unsigned consensus_min_q = 10;   // --consensus-min-q
  std::string dump_consensus;  // --dump-consensus-input (development: what -C hands to the GPU, then stop, no GPU)
  bool optical = false;        // -O given (not in the reference): the duplicates of every cluster are split into optical and other ones
  uint32_t optical_distance = 0;   // -O
  std::string dump_positions;  // --dump-positions (development: the -O positions of pass 1, then stop, no GPU)
  bool paired = false;         // -P (not in the reference): strand-symmetric words -- R1/R2 exchanged is the same molecule
  bool duplex = false;         // -D (not in the reference; needs -P): every kept record carries the duplex consensus of its cluster
  unsigned duplex_strand_cap = 40;   // --duplex-strand-cap
  bool chunked = false;        // --chunk-reads given (not in the reference): the device part runs as an accumulated run over chunks
  unsigned long long chunk_reads = 0;   // --chunk-reads: records per chunk
  bool bchunked = false;       // --chunk-barcoded given (not in the reference): a run with a barcode whose device part runs over chunks
  unsigned long long bchunk_reads = 0;  // --chunk-barcoded: records per chunk
  bool barcode_opts_given = false;    // --barcode-min-odds was given (--long-words refuses every --barcode-* flag)
  bool long_words = false;     // --long-words (the reference takes any -n): words of up to 512 nucleotides, ceil(n / 32) uint64 each, through humid_dedup_run_long
};

void usage(const char *argv0) {
  std::fprintf(stderr,
               "usage: %s [-n 24] [-m 1] [-l /dev/stderr] [-d .] [-s] [-q] [-a] [-e] [-x] [-g 1] [-b K [-w FILE ... | --cells-expected N] [--barcode-posterior]] [--word-pattern P] [-Q] [-C] [-O D] [-P [-D]] [--chunk-reads N] [--chunk-barcoded N] [--long-words] files...\n"
               "Deduplicate a dataset.\n"
               "  -n  word length\n  -m  allowed mismatches\n  -l  log file name\n  -d  output directory\n"
               "  -s  calculate statistics\n  -q  write deduplicated FastQ files (flag turns it OFF)\n"
               "  -a  write annotated FastQ files\n  -e  use edit distance (Levenshtein neighbours)\n"
               "  -x  use maximum clustering method\n"
               "  -g  GPUs to shard the read set over (1..16; default 1 or $HUMID_GPUS)\n"
               "  -b  barcode length K (1..32, K < n): the first K nucleotides of the word are matched exactly,\n"
               "      -m / -e / -x apply to the remaining n - K (reads are deduplicated per barcode; one GPU);\n"
               "      with -s also groups.dat: one line \"<barcode> <reads> <unique> <clusters>\" per barcode\n"
               "  -w  whitelist FILE for -b: plain text, one barcode of K letters per line (a trailing -1 is dropped, lines\n"
               "      starting with # are skipped).  A barcode that is not listed but has exactly one listed barcode one\n"
               "      substitution away becomes that barcode; reads whose barcode has several or none are left out like\n"
               "      reads with an N; with -s also barcodes.dat: exact / corrected / ambiguous / unmatched reads\n"
               "      -w A -w B -w C: a barcode of several segments (SPLiT-seq, inDrop, BD Rhapsody, sci-RNA-seq), one list per\n"
               "      segment in order.  All lines of a file have one length, that of its segment (1..10 letters, 8 files at most),\n"
               "      and the lengths add up to K.  Every segment is corrected on its own against its list, one substitution at the\n"
               "      most in each; --barcode-max-inexact N (default: all segments) leaves out reads with more than N segments\n"
               "      that are not exact.  barcodes.dat gains segment<s>.exact / .corrected / .ambiguous / .unmatched and\n"
               "      inexact<m> (reads with m such segments); a log line.  Not with --barcode-posterior or --cells-*\n"
               "  --word-pattern P  which letters of the FIRST file's read make the word, as UMI-tools' --bc-pattern: P is a\n"
               "      string of C (barcode), N (UMI) and X (skipped), one letter per nucleotide of the read.  The C letters in\n"
               "      order are the barcode and start the word (their number is K: -b may be left out), the N letters follow,\n"
               "      and the remaining n - #C - #N nucleotides come from the other files (with one file n = #C + #N).  A read\n"
               "      shorter than the pattern is left out like a read with an N.  Works with one -w, several or none; not with\n"
               "      a UMI in the headers, -P, -g or --barcode-posterior\n"
               "  --barcode-posterior  with -w: a barcode with SEVERAL listed barcodes one substitution away is decided as Cell\n"
               "      Ranger and STARsolo (1MM_multi) do: every candidate weighs (its exact reads in this input + 1) times the\n"
               "      error probability of the differing base (its quality, the first K letters of the first file's quality\n"
               "      line; at most Phred 40), and the heaviest wins when it weighs at least --barcode-min-odds N (default 39:\n"
               "      a posterior of 0.975; N >= 1) times all the others together.  The barcode must come from the first\n"
               "      file's read (no UMI in the headers, K nucleotides or more taken from it).  barcodes.dat gains the\n"
               "      lines multi (reads with several candidates) and rescued (those of them corrected); a log line\n"
               "  --cells-top N | --cells-expected N | --cells-min-reads N  with -b and without -w: the whitelist is taken from\n"
               "      the data.  The reads per barcode are counted and the cells are the N barcodes with the most reads (ties to\n"
               "      the smaller barcode), or every barcode with at least a tenth of the reads of the barcode at rank\n"
               "      (N + 50) / 100 (the order-of-magnitude rule of Cell Ranger 2 for N expected cells), or every barcode with\n"
               "      at least N reads.  --cells-merge-ratio R (default 0: off) then drops a cell one substitution away from a\n"
               "      cell with at least R times its reads.  Everything else is the -w path with the cells as the whitelist\n"
               "      (--barcode-posterior included); no cell found: exit 1.  A log line; with -s also cells.dat, one line\n"
               "      \"<barcode> <reads>\" per cell, and barcode_rank.dat, one line \"<reads> <barcodes>\" per number of reads.\n"
               "      One GPU; not with -P or -g\n"
               "  -Q  keep the record with the best base qualities of every cluster instead of the first one: among the\n"
               "      records that carry the cluster's most abundant word, the one with the largest sum of Phred qualities\n"
               "      >= 15 over all input files (Picard's SUM_OF_BASE_QUALITIES; ties: the first; one GPU).  Only the\n"
               "      _dedup files change\n"
               "  -C  write consensus reads: the sequence and quality lines of every kept record are replaced by the\n"
               "      consensus of all reads of its cluster, file by file: per column the base with the largest sum of\n"
               "      Phred qualities, the margin to the second largest as its quality (at most 93), N and ! on a tie;\n"
               "      bases below --consensus-min-q N (default 10) and letters outside ACGT do not vote.  Record lengths\n"
               "      do not change; only the _dedup files change; one GPU, inputs held in memory (no CRLF files)\n"
               "  -O  count optical duplicates within D pixels: records of one cluster on the same lane and tile whose x and\n"
               "      y both differ by at most D, chains of such records taken as one group (names of the first file as\n"
               "      @inst:run:flowcell:lane:tile:x:y; the file is taken to be ONE flowcell; records without such a name\n"
               "      have no position).  Every group counts all its records but one -- the cluster's kept record where\n"
               "      the group holds it -- as optical.  A log line, and with -s optical.dat; no other output changes; one GPU\n"
               "  -P  strand-symmetric (duplex) deduplication of exactly two files R1 R2, no UMI in the headers, even -n: a\n"
               "      pair and the pair with R1 and R2 exchanged (the same molecule read from its other strand) are one word,\n"
               "      and -m allows its mismatches against either orientation.  One record pair per cluster is kept; -a\n"
               "      appends :<id>/A to a record read as given, :<id>/B to one read exchanged, :0 to an unusable one; a log\n"
               "      line, and with -s strands.dat: clusters with reads of both orientations (duplex) and of one only.\n"
               "      Works with -x, -Q, -O, -D, -a, -s; not with -b, -w, -g, -e, -C (-D is the consensus of a -P run); one GPU\n"
               "  -D  with -P: write duplex consensus reads.  The records of a cluster that were read in the orientation of its\n"
               "      kept record vote with their read of the same file, the records read exchanged vote with their read of\n"
               "      the other file; each orientation makes a call of its own, as -C does, with a quality of at most\n"
               "      --duplex-strand-cap N (1..93, default 40); two calls of one base add their qualities, two calls of\n"
               "      different bases subtract them (N and ! when nothing is left).  --consensus-min-q applies.  Only the _dedup\n"
               "      files change; a log line, and with -s duplex.dat; inputs held in memory (no CRLF files); not with -C\n"
               "  --chunk-reads N  the GPU sees the records N at a time (N >= 1): every chunk's words are counted and merged into one\n"
               "      accumulated list, the list is clustered once, and every chunk is then given its results.  All outputs are\n"
               "      those of the run without the flag; the device holds one chunk and the distinct words, not the whole read\n"
               "      set.  Works with -n, -m, -e, -x, -s, -a, -q; one GPU; not with -g, -b, -w, --cells-*, --word-pattern, -P, -Q,\n"
               "      -C, -D or -O.  The host still holds all words at once: its limit of 2^31 - 1 records stays\n"
               "  --chunk-barcoded N  the same for a run with a barcode (-b K, or a --word-pattern with C letters): the GPU sees the\n"
               "      records N at a time (N >= 1).  With --cells-* a first pass over the chunks counts the barcodes and selects the\n"
               "      cells; with --barcode-posterior a pass adds up the reads per whitelist barcode; then every chunk's barcodes are\n"
               "      corrected and its (barcode, word) entries merged into one accumulated list, the list is clustered once, and\n"
               "      every chunk is given its results.  All outputs are those of the run without the flag.  Works with -n, -m, -e,\n"
               "      -x, -s, -a, -q, -b, -w (one or several), --barcode-max-inexact, --barcode-posterior, --barcode-min-odds,\n"
               "      --cells-* and --word-pattern; the word behind the barcode has at most 32 letters; one GPU; not with -g,\n"
               "      --chunk-reads, -P, -Q, -C, -D or -O\n"
               "  --long-words  word lengths up to 512 (-n 1 .. 512; without the flag 64 is the limit): a word takes ceil(n / 32)\n"
               "      uint64 and the GPU runs the long-word path for every n.  Outputs are those of the run without the flag\n"
               "      where both apply.  Works with -n, -m, -x, -d, -l, -s, -a, -q; one GPU; not with -e, -g, -b, -w, -P, -Q, -C, -D,\n"
               "      -O, --chunk-reads, --chunk-barcoded, --cells-*, --word-pattern or --barcode-*\n",
               argv0);
}

bool parse(int argc, char **argv, Args &a) {
  for (int i = 1; i < argc; i++) {
    std::string t = argv[i];
    auto need = [&](const char *what) -> const char * {
      if (i + 1 >= argc) { std::fprintf(stderr, "humid: %s needs a value\n", what); return nullptr; }
      return argv[++i];
    };
    if (t == "-h" || t == "--help") { usage(argv[0]); std::exit(0); }
    else if (t == "-n") { const char *v = need("-n"); if (!v) return false; a.word_length = std::strtoull(v, nullptr, 10); }
    else if (t == "-m") { const char *v = need("-m"); if (!v) return false; a.distance = std::strtoull(v, nullptr, 10); }
    else if (t == "-l") { const char *v = need("-l"); if (!v) return false; a.log_name = v; }
    else if (t == "-d") { const char *v = need("-d"); if (!v) return false; a.dir_name = v; }
    else if (t == "-g") { const char *v = need("-g"); if (!v) return false; a.gpus = (unsigned)std::strtoul(v, nullptr, 10); }
    else if (t == "-b") { const char *v = need("-b"); if (!v) return false; a.keyed = true; a.barcode = std::strtoull(v, nullptr, 10); }
    else if (t == "-w") { const char *v = need("-w"); if (!v) return false; a.whitelists.push_back(v); }
    else if (t == "--word-pattern") { const char *v = need("--word-pattern"); if (!v) return false; a.word_pattern = v; }
    else if (t == "--barcode-max-inexact") {
      const char *v = need("--barcode-max-inexact");
      if (!v) return false;
      char *end = nullptr;
      a.max_inexact = std::strtoull(v, &end, 10);
      if (*v < '0' || *v > '9' || *end != 0 || a.max_inexact > 8) {
        std::fprintf(stderr, "humid: --barcode-max-inexact takes a number of segments, 0 .. 8\n");
        return false;
      }
      a.max_inexact_given = true;
    }
    else if (t == "--barcode-posterior") a.posterior = !a.posterior;
    else if (t == "--barcode-min-odds") {
      const char *v = need("--barcode-min-odds");
      if (!v) return false;
      char *end = nullptr;
      a.min_odds = std::strtoull(v, &end, 10);
      a.barcode_opts_given = true;
      if (*v < '0' || *v > '9' || *end != 0 || a.min_odds < 1 || a.min_odds > 0xffffffffull) {
        std::fprintf(stderr, "humid: --barcode-min-odds takes odds of 1 .. 4294967295\n");
        return false;
      }
    }
    else if (t == "--cells-top" || t == "--cells-expected" || t == "--cells-min-reads" || t == "--cells-merge-ratio") {
      const char *v = need(t.c_str());
      if (!v) return false;
      char *end = nullptr;
      const unsigned long long x = std::strtoull(v, &end, 10);
      const bool ratio = t == "--cells-merge-ratio";
      if (*v < '0' || *v > '9' || *end != 0 || (ratio ? x > 0xffffffffull : x < 1)) {
        std::fprintf(stderr, ratio ? "humid: %s takes a ratio of 0 .. 4294967295\n" : "humid: %s takes a number of 1 or more\n", t.c_str());
        return false;
      }
      if (ratio) { a.cells_ratio_given = true; a.cells_ratio = x; }
      else {
        a.cells_mode = t == "--cells-top" ? (int)HUMID_CELLS_TOP : t == "--cells-expected" ? (int)HUMID_CELLS_EXPECTED : (int)HUMID_CELLS_MIN_READS;
        a.cells_param = x;
        a.cells_modes_given++;
      }
    }
    else if (t == "--dump-barcode-quals") { const char *v = need("--dump-barcode-quals"); if (!v) return false; a.dump_bc_quals = v; }
    else if (t == "--dump-words") { const char *v = need("--dump-words"); if (!v) return false; a.dump_words = v; }
    else if (t == "--dump-scores") { const char *v = need("--dump-scores"); if (!v) return false; a.dump_scores = v; }
    else if (t == "--dump-consensus-input") { const char *v = need("--dump-consensus-input"); if (!v) return false; a.dump_consensus = v; }
    else if (t == "--consensus-min-q") { const char *v = need("--consensus-min-q"); if (!v) return false; a.consensus_min_q = (unsigned)std::strtoul(v, nullptr, 10); }
    else if (t == "--duplex-strand-cap") { const char *v = need("--duplex-strand-cap"); if (!v) return false; a.duplex_strand_cap = (unsigned)std::strtoul(v, nullptr, 10); }
    else if (t == "--dump-positions") { const char *v = need("--dump-positions"); if (!v) return false; a.dump_positions = v; }
    else if (t == "-O") {
      const char *v = need("-O");
      if (!v) return false;
      char *end = nullptr;
      const unsigned long long d = std::strtoull(v, &end, 10);
      if (*v < '0' || *v > '9' || *end != 0 || d > 0xffffffffull) { std::fprintf(stderr, "humid: -O takes a distance of 0 .. 4294967295 pixels\n"); return false; }
      a.optical = true;
      a.optical_distance = (uint32_t)d;
    }
    else if (t == "--chunk-reads") {
      const char *v = need("--chunk-reads");
      if (!v) return false;
      char *end = nullptr;
      a.chunk_reads = std::strtoull(v, &end, 10);
      if (*v < '0' || *v > '9' || *end != 0) { std::fprintf(stderr, "humid: --chunk-reads takes a number of records, 1 or more\n"); return false; }
      a.chunked = true;
    }
    else if (t == "--chunk-barcoded") {
      const char *v = need("--chunk-barcoded");
      if (!v) return false;
      char *end = nullptr;
      a.bchunk_reads = std::strtoull(v, &end, 10);
      if (*v < '0' || *v > '9' || *end != 0) { std::fprintf(stderr, "humid: --chunk-barcoded takes a number of records, 1 or more\n"); return false; }
      a.bchunked = true;
    }
    else if (t == "--long-words") a.long_words = !a.long_words;
    else if (t == "-P") a.paired = !a.paired;
    else if (t == "-D") a.duplex = !a.duplex;
    else if (t == "-Q") a.best = !a.best;
    else if (t == "-C") a.consensus = !a.consensus;
    else if (t == "-s") a.stats = !a.stats;
    else if (t == "-q") a.filter = !a.filter;
    else if (t == "-a") a.annotate = !a.annotate;
    else if (t == "-e") a.edit = !a.edit;
    else if (t == "-x") a.maximum = !a.maximum;
    else if (t.size() > 1 && t[0] == '-') { std::fprintf(stderr, "humid: unknown option %s\n", t.c_str()); return false; }
    else a.files.push_back(t);
  }
  if (a.files.empty()) { std::fprintf(stderr, "humid: no input files\n"); return false; }
  return true;
}

// src/log.cc:4-15
time_t start_message(std::ofstream &log, const char *msg) {
  log << msg << "... ";
  log.flush();
  return time(nullptr);
}
void end_message(std::ofstream &log, time_t start) {
  time_t seconds = (time_t)difftime(time(nullptr), start);
  log << "done. (" << seconds / 60 << 'm' << seconds % 60 << "s)\n";
  log.flush();
}

// histogram `which` of the context as (key, value) pairs; HUMID_OK or the library's code
int fetch_hist(humid_ctx *ctx, uint32_t which, std::vector<std::pair<uint64_t, uint64_t>> &out) {
  uint64_t n = 0;
  int rc = humid_get_histogram(ctx, which, nullptr, nullptr, 0, &n);
  std::vector<uint64_t> k(n ? n : 1), v(n ? n : 1);
  if (rc == HUMID_OK && n) rc = humid_get_histogram(ctx, which, k.data(), v.data(), n, &n);
  out.clear();
  for (uint64_t i = 0; rc == HUMID_OK && i < n; i++) out.emplace_back(k[i], v[i]);
  return rc;
}

void make_dirs(const std::string &path) {   // std::filesystem::create_directories
  std::string cur;
  for (size_t i = 0; i <= path.size(); i++) {
    if (i == path.size() || path[i] == '/') {
      if (!cur.empty()) mkdir(cur.c_str(), 0777);
    }
    if (i < path.size()) cur.push_back(path[i]);
  }
}

// 1 = written, 0 = the library failed (humid_last_error says why), -1 = the file could not be written
int write_hist(humid_ctx *ctx, uint32_t which, const std::string &path) {
  std::vector<std::pair<uint64_t, uint64_t>> h;
  if (fetch_hist(ctx, which, h) != HUMID_OK) return 0;
  std::ofstream out(path, std::ios::out | std::ios::binary);
  for (const auto &kv : h) out << kv.first << ' ' << kv.second << '\n';   // src/humid.cc:333-349
  out.close();
  return out.fail() ? -1 : 1;
}

// -b K with -s: groups.dat, one line per distinct barcode in ascending order: "<barcode> <reads> <unique> <clusters>",
// the barcode as its K letters (first nucleotide first); the table comes reduced from the device
// (humid_get_group_stats).  Returns like write_hist.
struct GroupsTable {
  uint64_t n = 0;
  std::vector<uint64_t> key, reads;
  std::vector<uint32_t> leaf_off, cluster_off;
};
// (apart from the writing: an accumulated run answers only until its first map)
int fetch_groups(humid_ctx *ctx, GroupsTable &t) {
  uint64_t n = 0, nk = 0;
  if (humid_get_group_stats(ctx, 0, &n, nullptr, nullptr, nullptr, nullptr) != HUMID_OK) return 0;
  t.key.assign(n ? n : 1, 0);
  t.reads.assign(n ? n : 1, 0);
  t.leaf_off.assign(n + 1, 0);
  t.cluster_off.assign(n + 1, 0);
  if (humid_get_group_stats(ctx, n, &n, t.reads.data(), t.leaf_off.data(), t.cluster_off.data(), nullptr) != HUMID_OK) return 0;
  if (humid_get_group_keys(ctx, t.key.data(), n, &nk) != HUMID_OK) return 0;
  if (nk != n) return -1;
  t.n = n;
  return 1;
}
int write_groups(const GroupsTable &t, size_t barcode_nt, const std::string &path) {
  std::ofstream out(path, std::ios::out | std::ios::binary);
  std::string letters(barcode_nt, 'A');
  for (uint64_t g = 0; g < t.n; g++) {
    for (size_t i = 0; i < barcode_nt; i++) letters[i] = "ACGT"[(t.key[g] >> (2 * (barcode_nt - 1 - i))) & 3];
    out << letters << ' ' << t.reads[g] << ' ' << t.leaf_off[g + 1] - t.leaf_off[g] << ' ' << t.cluster_off[g + 1] - t.cluster_off[g] << '\n';
  }
  out.close();
  return out.fail() ? -1 : 1;
}

// --cells-* with -s: cells.dat, one line "<barcode> <reads>" per cell in ascending order, the barcode as its K letters, and
// barcode_rank.dat, one line "<reads> <barcodes>" per number of reads a barcode has, ascending (humid_get_discovered_cells,
// humid_get_barcode_count_hist).  Returns like write_hist.
int write_cells(humid_ctx *ctx, size_t barcode_nt, const std::string &cells_path, const std::string &rank_path) {
  uint64_t n = 0, h = 0;
  if (humid_get_discovered_cells(ctx, nullptr, nullptr, 0, &n) != HUMID_OK) return 0;
  std::vector<uint64_t> bc(n ? n : 1);
  std::vector<uint32_t> reads(n ? n : 1);
  if (n && humid_get_discovered_cells(ctx, bc.data(), reads.data(), n, &n) != HUMID_OK) return 0;
  if (humid_get_barcode_count_hist(ctx, nullptr, nullptr, 0, &h) != HUMID_OK) return 0;
  std::vector<uint64_t> hk(h ? h : 1), hv(h ? h : 1);
  if (h && humid_get_barcode_count_hist(ctx, hk.data(), hv.data(), h, &h) != HUMID_OK) return 0;
  std::ofstream out(cells_path, std::ios::out | std::ios::binary);
  std::string letters(barcode_nt, 'A');
  for (uint64_t g = 0; g < n; g++) {
    for (size_t i = 0; i < barcode_nt; i++) letters[i] = "ACGT"[(bc[g] >> (2 * (barcode_nt - 1 - i))) & 3];
    out << letters << ' ' << reads[g] << '\n';
  }
  out.close();
  if (out.fail()) return -1;
  std::ofstream rank(rank_path, std::ios::out | std::ios::binary);
  for (uint64_t i = 0; i < h; i++) rank << hk[i] << ' ' << hv[i] << '\n';
  rank.close();
  return rank.fail() ? -1 : 1;
}

// -w FILE: one barcode of barcode_nt letters per line -> packed like the words (first letter most significant).
// Trailing whitespace and CR are dropped, then a trailing "-1" (10x style); empty lines and lines starting with '#'
// are skipped; letters in either case.  false + a one-line message in err when the file cannot serve.
// barcode_nt = 0 (one file of several: a segment's list): the first barcode's length is taken, returned in barcode_nt,
// and every other line must have it.
bool read_whitelist(const std::string &path, size_t &barcode_nt, std::vector<uint64_t> &out, std::string &err) {
  const bool infer = barcode_nt == 0;
  const size_t before = out.size();
  if (path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0) {
    err = "-w takes a plain text file, not " + path + " (decompress it first)";
    return false;
  }
  std::ifstream in(path, std::ios::in | std::ios::binary);
  if (!in) { err = "-w: cannot open " + path; return false; }
  std::string line;
  size_t ln = 0;
  while (std::getline(in, line)) {
    ln++;
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    if (line.size() >= 2 && line.compare(line.size() - 2, 2, "-1") == 0) line.resize(line.size() - 2);
    if (infer && barcode_nt == 0) barcode_nt = line.size();
    if (line.size() != barcode_nt) {
      err = "-w: " + path + " line " + std::to_string(ln) + " has " + std::to_string(line.size()) + " letters, " +
            (infer ? "the lines before it " : "-b says ") + std::to_string(barcode_nt);
      return false;
    }
    if (infer && barcode_nt > 10) {
      err = "-w: " + path + " holds barcodes of " + std::to_string(barcode_nt) + " letters: a segment of several -w has 1 .. 10";
      return false;
    }
    uint64_t v = 0;
    for (char ch : line) {
      uint64_t x;
      switch (ch) {
        case 'A': case 'a': x = 0; break;
        case 'C': case 'c': x = 1; break;
        case 'G': case 'g': x = 2; break;
        case 'T': case 't': x = 3; break;
        default:
          err = "-w: " + path + " line " + std::to_string(ln) + " has a letter outside ACGT";
          return false;
      }
      v = (v << 2) | x;
    }
    out.push_back(v);
  }
  if (in.bad()) { err = "-w: reading " + path + " failed"; return false; }
  if (out.size() == before) { err = "-w: " + path + " holds no barcode"; return false; }
  return true;
}

// -Q: the score of a record is Picard's SUM_OF_BASE_QUALITIES over its quality lines in all input files: the sum of
// q = byte - 33 over the bytes with q >= 15 (a line terminator never counts: '\r' and '\n' are below 33 + 15)
inline uint64_t quality_sum(const char *q, size_t n) {
  uint64_t t = 0;
  for (size_t i = 0; i < n; i++) {
    const unsigned v = (unsigned char)q[i];
    t += v >= 48u ? v - 33u : 0u;
  }
  return t;
}
inline uint32_t clamp_score(uint64_t t) { return t > 0xffffffffull ? 0xffffffffu : (uint32_t)t; }

// -C: one layer of reads as humid_consensus takes it -- the sequence lines of a mapped file in one blob, its quality
// lines in another, off[i] .. off[i + 1] the bytes of record i in both (a record whose two lines differ in length
// gives the shorter one)
void gather_layer(const MappedFastq &m, size_t n, unsigned threads, std::vector<uint64_t> &off, std::vector<uint8_t> &b,
                  std::vector<uint8_t> &q) {
  off.assign(n + 1, 0);
  parallel_ranges(n, threads, [&](size_t lo, size_t hi, unsigned) {
    std::string_view nm, sq, st, ql;
    for (size_t i = lo; i < hi; i++) {
      m.lines(i, nm, sq, st, ql);
      off[i + 1] = sq.size() < ql.size() ? sq.size() : ql.size();
    }
  });
  for (size_t i = 0; i < n; i++) off[i + 1] += off[i];
  b.resize(off[n]);
  q.resize(off[n]);
  parallel_ranges(n, threads, [&](size_t lo, size_t hi, unsigned) {
    std::string_view nm, sq, st, ql;
    for (size_t i = lo; i < hi; i++) {
      m.lines(i, nm, sq, st, ql);
      const size_t len = (size_t)(off[i + 1] - off[i]);
      if (len) { memcpy(&b[off[i]], sq.data(), len); memcpy(&q[off[i]], ql.data(), len); }
    }
  });
}

// Plain (uncompressed) output of the fast path, written through a shared mapping of the output file:
// every worker copies its share of the records straight to their final place, so the page cache is
// filled by all cores at once (one writer through pwrite() is bound by a single core's copy rate,
// parallel pwrite()s into one file serialise on the inode lock).  size_of(i) = bytes record i
// contributes (0: not written), emit(i, q) writes them at q and returns the end.
// Returns 1 = written, 0 = not possible on this file (the caller takes the buffered writer), -1 = failed.
int write_mapped(const std::string &path, size_t n, unsigned threads, const std::function<size_t(size_t)> &size_of,
                 const std::function<char *(size_t, char *)> &emit) {
  if (threads == 0) threads = 1;
  const bool timing = getenv("HUMID_TIMING") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  const auto t_begin = now();
  std::vector<uint64_t> part(threads + 1, 0);
  parallel_ranges(n, threads, [&](size_t b, size_t e, unsigned w) {
    uint64_t t = 0;
    for (size_t i = b; i < e; i++) t += size_of(i);
    part[w + 1] = t;
  });
  const auto t_sized = now();
  const bool one = threads <= 1 || n < 4096;            // parallel_ranges ran everything as worker 0
  for (unsigned w = 0; w < threads; w++) part[w + 1] += part[w];
  const uint64_t total = part[threads];
  const int fd = ::open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) return -1;
  if (total == 0) return ::close(fd) == 0 ? 1 : -1;
  // the blocks are reserved first, so a full disk is an error code here and not a SIGBUS later.
  // (Measured and rejected: extending the file sparsely and letting the workers' page faults
  // allocate it -- on tmpfs parallel faults into one file contend so badly that pass 2 takes 3x
  // longer than with the single-threaded allocation of posix_fallocate.)
  // (Also measured and rejected, end of round 3: reserving in 32 MB chunks on a thread of its own while the workers
  // copy behind it -- the allocation and the faults on the same file slow each other down: 100-190 ms for both
  // together against 45 + 50-120 one after the other.)
  if (posix_fallocate(fd, 0, (off_t)total) != 0) { ::close(fd); return 0; }      // e.g. a device: buffered writer
  const auto t_alloc = now();
  char *m = (char *)mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  if (m == (char *)MAP_FAILED) { ::close(fd); return 0; }
  parallel_ranges(n, threads, [&](size_t b, size_t e, unsigned w) {
    char *const q0 = m + (one ? 0 : part[w]);
    char *q = q0;
    // (measured and rejected, end of round 3: MADV_POPULATE_WRITE over the worker's range in front of the copy -- the
    // copy phase is bound by the 200 k write faults of a 0.8 GB file, 50-120 ms against ~45 ms of preallocation, and
    // populating the same pages in one call per worker was no faster: 115-130 ms)
    for (size_t i = b; i < e; i++) q = emit(i, q);
    // this worker's pages leave the address space here, in parallel (the data stays in the page cache:
    // the mapping is shared); the munmap below then has next to nothing to walk
    const uintptr_t lo = ((uintptr_t)q0 + 4095) & ~(uintptr_t)4095, hi = (uintptr_t)q & ~(uintptr_t)4095;
    if (hi > lo) madvise((void *)lo, hi - lo, MADV_DONTNEED);
  });
  const auto t_copied = now();
  const bool ok = munmap(m, total) == 0;
  const bool closed = ::close(fd) == 0;
  if (timing)
    std::fprintf(stderr, "[humid]   mapped write of %.2f GB with %u workers: sizes %.1f ms, preallocation %.1f ms, copy %.1f ms, unmap + close %.1f ms\n",
                 (double)total / 1e9, threads, ms(t_begin, t_sized), ms(t_sized, t_alloc), ms(t_alloc, t_copied), ms(t_copied, now()));
  return (closed && ok) ? 1 : -1;
}

}  // namespace

int main(int argc, char **argv) {
  // development aid (no GPU): --gunzip IN.gz OUT inflates through the host's own decoder only
  // (fast_inflate.hpp); exit code 3 = the decoder declined the file
  if (argc == 4 && std::string(argv[1]) == "--gunzip") {
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) return 1;
    std::string z((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    struct Buf { std::vector<char> v; size_t limit; } buf;
    buf.limit = z.size() * 1100 + (1u << 20);            // DEFLATE cannot expand more than 1032 : 1
    if (buf.limit > ((size_t)8 << 30)) buf.limit = (size_t)8 << 30;
    auto grow = [](void *user, size_t min_cap, size_t *cap) -> char * {
      Buf *b = (Buf *)user;
      if (min_cap > b->limit) return nullptr;
      if (b->v.size() < min_cap) b->v.resize(min_cap);
      *cap = b->v.size();
      return b->v.data();
    };
    size_t n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = humid_host::fast_gunzip((const uint8_t *)z.data(), z.size(), grow, &buf, &n, host_threads());
    if (getenv("HUMID_TIMING"))
      std::fprintf(stderr, "fast_gunzip: %zu -> %zu bytes in %.3f s\n", z.size(), n,
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    if (!ok) return 3;
    std::ofstream out(argv[3], std::ios::binary);
    out.write(buf.v.data(), (std::streamsize)n);
    return out ? 0 : 1;
  }
  if (getenv("HUMID_TIMING")) {
    timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    std::fprintf(stderr, "[humid] main() entered at %.6f (epoch s)\n", (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec);
  }
  Args a;
  if (!parse(argc, argv, a)) { usage(argv[0]); return 2; }
  if (a.word_length == 0 || a.word_length > (a.long_words ? (size_t)HUMID_LONG_MAX_NT : 64)) {
    if (a.long_words) std::fprintf(stderr, "humid: word length %zu is not supported by the HIP path (1..%u with --long-words)\n", a.word_length, HUMID_LONG_MAX_NT);
    else std::fprintf(stderr, "humid: word length %zu is not supported by the HIP path (1..64; --long-words takes 1..%u)\n", a.word_length, HUMID_LONG_MAX_NT);
    return 2;
  }
  if (a.gpus == 1 && getenv("HUMID_GPUS")) a.gpus = (unsigned)std::strtoul(getenv("HUMID_GPUS"), nullptr, 10);
  if (a.long_words) {
    // what a long-word run does not do: one line, before anything is opened and before any GPU use
    const char *why = nullptr;
    if (a.edit) why = "--long-words does not work with -e (Hamming neighbours only)";
    else if (a.gpus != 1 || getenv("HUMID_FORCE_SHARDED")) why = "--long-words runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)";
    else if (a.keyed) why = "--long-words does not work with -b";
    else if (!a.whitelists.empty()) why = "--long-words does not work with -w";
    else if (a.paired) why = "--long-words does not work with -P";
    else if (a.best) why = "--long-words does not work with -Q";
    else if (a.consensus) why = "--long-words does not work with -C";
    else if (a.duplex) why = "--long-words does not work with -D";
    else if (a.optical) why = "--long-words does not work with -O";
    else if (a.chunked) why = "--long-words does not work with --chunk-reads";
    else if (a.bchunked) why = "--long-words does not work with --chunk-barcoded";
    else if (a.cells_mode >= 0 || a.cells_ratio_given) why = "--long-words does not work with --cells-top / --cells-expected / --cells-min-reads / --cells-merge-ratio";
    else if (!a.word_pattern.empty()) why = "--long-words does not work with --word-pattern";
    else if (a.posterior || a.max_inexact_given || a.barcode_opts_given) why = "--long-words does not work with --barcode-posterior / --barcode-min-odds / --barcode-max-inexact";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 2; }
  }
  if (a.gpus < 1 || a.gpus > 16) {
    std::fprintf(stderr, "humid: -g takes 1 .. 16 GPUs\n");
    return 2;
  }
  // HUMID_FORCE_SHARDED=1: the rank orchestration also for -g 1 (one rank; exercises the transport)
  const bool sharded = a.gpus > 1 || getenv("HUMID_FORCE_SHARDED") != nullptr;
  const bool discover = a.cells_mode >= 0;                 // the whitelist comes from the data
  if (a.bchunked) {
    // what a keyed accumulated run does not do, as far as the flags alone tell: one line, before anything is opened and
    // before any GPU use (the length of the word behind the barcode follows below, once --word-pattern is read)
    const char *why = nullptr;
    if (a.bchunk_reads == 0) why = "--chunk-barcoded takes a number of records, 1 or more";
    else if (a.chunked) why = "--chunk-barcoded does not work with --chunk-reads (the one is for runs with a barcode, the other for runs without)";
    else if (sharded) why = "--chunk-barcoded runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)";
    else if (!a.keyed && a.word_pattern.empty()) why = "--chunk-barcoded needs a barcode (-b K, or a --word-pattern with C letters); without one it is --chunk-reads";
    else if (a.paired) why = "--chunk-barcoded does not work with -P";
    else if (a.best) why = "--chunk-barcoded does not work with -Q (the post-run passes need a complete run)";
    else if (a.consensus) why = "--chunk-barcoded does not work with -C (the post-run passes need a complete run)";
    else if (a.duplex) why = "--chunk-barcoded does not work with -D";
    else if (a.optical) why = "--chunk-barcoded does not work with -O (the post-run passes need a complete run)";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 2; }
  }
  if (a.chunked) {
    // what an accumulated run does not do: one line, before anything is opened and before any GPU use
    const char *why = nullptr;
    if (a.chunk_reads == 0) why = "--chunk-reads takes a number of records, 1 or more";
    else if (sharded) why = "--chunk-reads runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)";
    else if (a.keyed) why = "--chunk-reads does not work with -b";
    else if (!a.whitelists.empty()) why = "--chunk-reads does not work with -w";
    else if (discover || a.cells_ratio_given) why = "--chunk-reads does not work with --cells-top / --cells-expected / --cells-min-reads / --cells-merge-ratio";
    else if (!a.word_pattern.empty()) why = "--chunk-reads does not work with --word-pattern";
    else if (a.paired) why = "--chunk-reads does not work with -P";
    else if (a.best) why = "--chunk-reads does not work with -Q (the post-run passes need a complete run)";
    else if (a.consensus) why = "--chunk-reads does not work with -C (the post-run passes need a complete run)";
    else if (a.duplex) why = "--chunk-reads does not work with -D";
    else if (a.optical) why = "--chunk-reads does not work with -O (the post-run passes need a complete run)";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 2; }
  }
  const bool segmented = a.whitelists.size() > 1;          // one -w per segment of the barcode
  // what --word-pattern and several -w do not work with: one line each, before anything is opened
  {
    const char *why = nullptr;
    if (!a.word_pattern.empty()) {
      if (a.paired) why = "--word-pattern does not work with -P (a strand-symmetric word takes the same letters of both reads)";
      else if (sharded) why = "--word-pattern runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)";
      else if (a.posterior) why = "--word-pattern does not work with --barcode-posterior (the barcode's qualities are taken from the start of the read)";
    }
    if (!why && segmented) {
      if (a.posterior) why = "--barcode-posterior does not work with several -w (a segment of the barcode is corrected without qualities)";
      else if (discover || a.cells_ratio_given) why = "--cells-top / --cells-expected / --cells-min-reads / --cells-merge-ratio do not work with several -w (the segments' lists are the whitelist)";
      else if (a.whitelists.size() > 8) why = "-w: a barcode has 8 segments at the most";
    }
    if (!why && a.max_inexact_given && !segmented) why = "--barcode-max-inexact needs several -w (it counts the segments of a barcode)";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 1; }
  }
  WordPlan pattern_plan;
  if (!a.word_pattern.empty()) {
    size_t n_c = 0;
    std::string err;
    if (!make_pattern_plan(a.word_pattern, a.files.size(), a.word_length, pattern_plan, n_c, err)) {
      std::fprintf(stderr, "humid: %s\n", err.c_str());
      return 1;
    }
    if (a.keyed && a.barcode != n_c) {
      std::fprintf(stderr, "humid: --word-pattern has %zu C letters, -b says %zu\n", n_c, a.barcode);
      return 1;
    }
    if (n_c) { a.keyed = true; a.barcode = n_c; }
    // the word is made of the reads' letters alone: a UMI in the headers would start it
    FastqReader peek(a.files.front());
    if (!peek.ok()) { std::fprintf(stderr, "humid: cannot open %s\n", a.files.front().c_str()); return 1; }
    FastqRecord r;
    if (peek.read(r) && !header_umi(r.name).empty()) {
      std::fprintf(stderr, "humid: --word-pattern takes the word from the reads alone: %s has a UMI in its headers\n", a.files.front().c_str());
      return 1;
    }
  }
  if (a.bchunked) {
    const char *why = nullptr;
    if (!a.keyed) why = "--chunk-barcoded needs a barcode (-b K, or a --word-pattern with C letters); without one it is --chunk-reads";
    else if (a.barcode < a.word_length && a.word_length - a.barcode > 32)
      why = "--chunk-barcoded takes a word of at most 32 letters behind the barcode (-n minus -b)";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 2; }
  }
  if (discover || a.cells_ratio_given) {
    const char *why = nullptr;
    if (a.cells_modes_given > 1) why = "--cells-top, --cells-expected and --cells-min-reads exclude each other (one rule selects the cells)";
    else if (!discover) why = "--cells-merge-ratio needs --cells-top, --cells-expected or --cells-min-reads (it merges the cells they select)";
    else if (!a.whitelists.empty()) why = "--cells-top / --cells-expected / --cells-min-reads do not work with -w (the whitelist comes from FILE or from the data)";
    else if (a.paired) why = "--cells-top / --cells-expected / --cells-min-reads do not work with -P";
    else if (sharded) why = "--cells-top / --cells-expected / --cells-min-reads run on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)";
    else if (!a.keyed) why = "--cells-top / --cells-expected / --cells-min-reads need -b K (the cells are barcodes of K letters)";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 2; }
  }
  if (a.keyed && (a.barcode < 1 || a.barcode > 32 || a.barcode >= a.word_length)) {
    std::fprintf(stderr, "humid: -b takes a barcode length of 1 .. 32 nucleotides below the word length (-n %zu)\n", a.word_length);
    return 2;
  }
  if (a.keyed && sharded) {
    std::fprintf(stderr, "humid: -b runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)\n");
    return 2;
  }
  if (a.best && sharded) {
    std::fprintf(stderr, "humid: -Q runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)\n");
    return 2;
  }
  if (a.consensus && sharded) {                          // (the reads of a cluster lie on several ranks)
    std::fprintf(stderr, "humid: -C runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)\n");
    return 1;
  }
  if (a.optical && sharded) {                            // (the reads of a cluster lie on several ranks)
    std::fprintf(stderr, "humid: -O runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)\n");
    return 1;
  }
  if (a.paired) {
    const char *why = nullptr;
    if (a.files.size() != 2) why = "-P takes exactly two input files (R1 and R2)";
    else if (a.word_length % 2 != 0) why = "-P needs an even word length (-n): half of the word comes from each file";
    else if (a.keyed) why = "-P does not work with -b";
    else if (!a.whitelists.empty()) why = "-P does not work with -w";
    else if (sharded) why = "-P runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)";
    else if (a.edit) why = "-P does not work with -e (edit distance against an exchanged pair is not defined here)";
    else if (a.consensus) why = "-P does not work with -C (the consensus of a -P run is -D: it takes half of the reads from the other file)";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 2; }
  }
  if (a.duplex) {
    const char *why = nullptr;
    if (a.consensus) why = "-D does not work with -C (-C is the consensus of a plain run, -D that of a -P run)";
    else if (!a.paired) why = "-D needs -P (the duplex consensus combines the two orientations of a strand-symmetric run)";
    else if (a.duplex_strand_cap < 1 || a.duplex_strand_cap > 93) why = "--duplex-strand-cap takes 1 .. 93";
    if (why) { std::fprintf(stderr, "humid: %s\n", why); return 2; }
  }
  if (a.consensus_min_q > 93) {
    std::fprintf(stderr, "humid: --consensus-min-q takes 0 .. 93\n");
    return 2;
  }
  const bool dump_only = !a.dump_words.empty() || !a.dump_scores.empty() || !a.dump_consensus.empty() || !a.dump_positions.empty() ||
                         !a.dump_bc_quals.empty();   // development: stop after pass 1, no GPU
  const bool cons_out = a.consensus || a.duplex;                            // pass 2 writes consensus bytes (put_consensus)
  const bool want_reads = cons_out || !a.dump_consensus.empty();         // the reads themselves are gathered from the mappings
  const bool scoring = a.best || !a.dump_scores.empty();                    // (without -Q pass 1 does no new work)
  const bool positions = a.optical || !a.dump_positions.empty();            // (nor without -O)
  std::vector<uint64_t> whitelist;
  std::vector<uint32_t> seg_nt;                            // several -w: the letters and the entries of every file's list,
  std::vector<uint64_t> seg_n;                             // the lists themselves one behind the other in whitelist
  if (!a.whitelists.empty()) {
    if (!a.keyed) {
      std::fprintf(stderr, "humid: -w needs -b K (the whitelist holds barcodes of K letters)\n");
      return 2;
    }
    std::string err;
    size_t total_nt = 0;
    for (const std::string &file : a.whitelists) {
      size_t nt = segmented ? 0 : a.barcode;
      const size_t before = whitelist.size();
      if (!read_whitelist(file, nt, whitelist, err)) {
        std::fprintf(stderr, "humid: %s\n", err.c_str());
        return 2;
      }
      seg_nt.push_back((uint32_t)nt);
      seg_n.push_back(whitelist.size() - before);
      total_nt += nt;
    }
    if (segmented && total_nt != a.barcode) {
      std::fprintf(stderr, "humid: -w: the segments of the %zu files add up to %zu letters, the barcode has %zu\n", a.whitelists.size(), total_nt,
                   a.barcode);
      return 2;
    }
    if (segmented && a.max_inexact_given && a.max_inexact > a.whitelists.size()) {
      std::fprintf(stderr, "humid: --barcode-max-inexact %llu exceeds the %zu segments\n", a.max_inexact, a.whitelists.size());
      return 2;
    }
  }
  const bool corrected = !whitelist.empty() || discover;
  if (a.posterior && !corrected) {
    std::fprintf(stderr, "humid: --barcode-posterior needs -w FILE (it decides between the listed barcodes near a read's barcode)\n");
    return 2;
  }
  const bool bc_quals = a.posterior || !a.dump_bc_quals.empty();            // pass 1 gathers the barcode's qualities
  if (bc_quals && !a.keyed) {
    std::fprintf(stderr, "humid: %s needs -b K (the qualities of the barcode's K nucleotides)\n", a.posterior ? "--barcode-posterior" : "--dump-barcode-quals");
    return 2;
  }
  std::ofstream log(a.log_name.c_str(), std::ios::out | std::ios::binary);

  // The HIP runtime and the context come up (a few hundred ms) while pass 1 parses the files.
  humid_ctx *ctx = nullptr;
  int ctx_rc = HUMID_OK;
  std::string ctx_err;
  struct Joiner {
    std::thread th;
    ~Joiner() { if (th.joinable()) th.join(); }
  } ctx_init;
  // ... and as soon as the number of reads is known (files indexed) it takes ONE slab of device
  // memory for the whole run (humid_ctx_reserve) while pass 1 is still gathering words.
  std::atomic<long long> n_known{-1};                   // -1: not yet; 0: no slab wanted
  uint8_t *pinned = nullptr;                            // written by the init thread, read after its join
  uint64_t pin_bytes = 0;
  // -g: the ranks (threads with a context, a stream and a communicator each) come up the same way
  std::unique_ptr<ShardedSession> ranks;
  if (!dump_only && sharded) ranks.reset(new ShardedSession(a.gpus));
  // (-C: the GPU is opened only once the inputs are known to be held in memory, see below)
  auto start_ctx = [&] {
    ctx_init.th = std::thread([&] {
      const auto ti = std::chrono::steady_clock::now();
      auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - ti).count(); };
      ctx_rc = humid_ctx_create(&ctx, -1, nullptr);
      if (ctx_rc != HUMID_OK) { ctx_err = humid_last_error(nullptr); return; }
      const double t_ctx = since();
      long long n;
      while ((n = n_known.load(std::memory_order_acquire)) < 0) std::this_thread::yield();
      const double t_wait = since();
      double t_pin = t_wait, t_slab = t_wait;
      if (n > 0) {
        // page-locked staging for what crosses PCIe: packed words + flags in, cluster ids + keep flags out
        const uint64_t wb = (uint64_t)n * (a.long_words ? 8 * ((a.word_length + 31) / 32) : a.word_length > 32 ? 16 : 8);
        pin_bytes = wb + (uint64_t)n + (uint64_t)n * 4 + (uint64_t)n + 64;
        std::thread pin_thread;                            // the two take ~30 ms and ~40 ms: side by side
        if (getenv("HUMID_NO_PINNED") == nullptr && !a.keyed)   // (-b: keys and shorter words, from ordinary memory)
          pin_thread = std::thread([&] { pinned = (uint8_t *)humid_host_alloc(pin_bytes); t_pin = since(); });
        if (getenv("HUMID_NO_SLAB") == nullptr)
          humid_ctx_reserve(ctx, a.chunked ? std::min<uint64_t>((uint64_t)n, a.chunk_reads) :
                                 a.bchunked ? std::min<uint64_t>((uint64_t)n, a.bchunk_reads) : (uint64_t)n,
                            (uint32_t)std::min<size_t>(a.word_length, 64));   // one slab (--chunk-reads: for one chunk) + the code object loaded
        t_slab = since();
        if (pin_thread.joinable()) pin_thread.join();
      }
      if (getenv("HUMID_TIMING"))
        std::fprintf(stderr, "[humid]   init thread: context %.3f s, read count known %.3f s, page-locked staging %.3f s, slab + code object %.3f s\n",
                     t_ctx, t_wait, t_pin, t_slab);
    });
  };
  if (!dump_only && !sharded && !cons_out) start_ctx();
  struct Release {                                      // every early return lets the thread go on
    std::atomic<long long> &n;
    ~Release() { long long e = -1; n.compare_exchange_strong(e, 0); }
  } release_init{n_known};
  const auto t_start = std::chrono::steady_clock::now();
  auto phase = [&](const char *what) {                 // HUMID_TIMING=1: wall time of the host phases
    if (getenv("HUMID_TIMING"))
      std::fprintf(stderr, "[humid] %-28s %.3f s\n", what,
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
  };

  // ---- preCompute (src/humid.cc:38-59): UMI size from the first header of the first file ----
  size_t first_umi = 0;
  {
    FastqReader peek(a.files.front());
    if (!peek.ok()) { std::fprintf(stderr, "humid: cannot open %s\n", a.files.front().c_str()); return 1; }
    FastqRecord r;
    if (peek.read(r)) first_umi = header_umi(r.name).size();   // empty file: no UMI (the reference crashes)
  }
  if (a.paired && first_umi != 0) {
    std::fprintf(stderr, "humid: -P takes the word from the two reads alone: %s has a UMI in its headers\n", a.files.front().c_str());
    return 2;
  }
  WordPlan plan = a.word_pattern.empty() ? make_plan(first_umi, a.files.size(), a.word_length) : pattern_plan;
  if (bc_quals && (plan.header_umi != 0 || plan.take[0] < a.barcode)) {
    // the barcode's qualities are the first K letters of the first file's quality line: the barcode must be its read's start
    const char *flag = a.posterior ? "--barcode-posterior" : "--dump-barcode-quals";
    if (plan.header_umi != 0)
      std::fprintf(stderr, "humid: %s: the headers of %s carry a UMI, which starts the word: the barcode has no base qualities\n", flag,
                   a.files.front().c_str());
    else
      std::fprintf(stderr, "humid: %s: only %zu nucleotides are taken from %s, fewer than the barcode's %zu (-b)\n", flag,
                   (size_t)plan.take[0], a.files.front().c_str(), a.barcode);
    return 2;
  }
  time_t t = start_message(log, "Determing nucleotides to take");
  end_message(log, t);
  log << "  header: " << plan.header_umi;
  for (size_t i = 0; i < a.files.size(); i++) log << "\n  " << a.files[i] << ": " << plan.take[i];
  log << "\n";

  // ---- fast path: plain canonical FastQ files are mapped and indexed on all cores ----
  const unsigned threads = host_threads();
  std::vector<MappedFastq> maps(a.files.size());
  bool fast = a.files.size() <= 64 && getenv("HUMID_HOST_SLOW") == nullptr;
  if (fast) {
    // one opener per file (a gzip file is inflated by one zlib stream); the indexing inside uses
    // the remaining workers
    const size_t nf = a.files.size();
    const size_t budget = retain_budget_bytes() / (nf ? nf : 1);
    const unsigned per = threads / (unsigned)nf ? threads / (unsigned)nf : 1;
    std::vector<char> okf(nf, 0);
    std::vector<std::thread> openers;
    for (size_t f = 0; f < nf; f++)
      openers.emplace_back([&, f] { okf[f] = maps[f].open(a.files[f], per, budget) ? 1 : 0; });
    for (auto &th : openers) th.join();
    for (size_t f = 0; f < nf; f++) fast = fast && okf[f];
  }

  phase("files opened / indexed");
  if (want_reads && !fast) {
    std::fprintf(stderr, "humid: %s needs the input files held in memory: not on the streaming input path (CRLF line ends, files over\n"
                         "       HUMID_RETAIN_GB, HUMID_HOST_SLOW), where the reads are not retained\n", a.duplex ? "-D" : "-C");
    return 1;
  }
  if (!dump_only && cons_out) start_ctx();
  // ---- pass 1: readData (src/humid.cc:89-100) ----
  t = start_message(log, "Reading data");
  const size_t wpr = a.long_words ? (a.word_length + 31) / 32 : a.word_length > 32 ? 2 : 1;   // uint64 per word (include/humid_hip.h)
  std::vector<uint64_t> words;
  std::vector<uint8_t> filtered;
  std::vector<uint8_t> bases;                      // device-side packing: word_length raw symbols per record
  // HUMID_DEVICE_PACK=1: the host only gathers the raw symbols and the GPU packs them
  // (humid_dedup_run_bases).  Not the default: 24 raw bytes per read instead of 9 packed ones cross
  // PCIe, which costs more than the host's packing saves (profiles/r02d_cli_e2e.txt).
  // (-Q: the selection compares the packed words, so the host packs them)
  const bool device_pack = fast && !dump_only && !sharded && !a.keyed && !a.best && !a.optical && !a.paired && !a.chunked && !a.long_words && getenv("HUMID_DEVICE_PACK") != nullptr;
  uint64_t n_records = 0;
  std::vector<uint32_t> scores;                    // -Q: one per record
  std::vector<uint32_t> pos_tile, pos_x, pos_y;    // -O: the position of every record (position.hpp)
  // --barcode-posterior: K quality bytes per record, the first K letters of the first file's quality line ('!' where
  // the line is shorter: such a read is filtered and its row never read)
  std::vector<uint8_t> bcq;
  const size_t K = a.barcode;
  auto put_bc_quals = [&](uint8_t *row, const char *q, size_t len) {
    const size_t have = len < K ? len : K;
    std::memcpy(row, q, have);
    std::memset(row + have, '!', K - have);
  };
  if (fast) {
    size_t n = maps[0].records();
    for (auto &m : maps) n = m.records() < n ? m.records() : n;     // stop at the shortest file
    n_records = n;
    n_known.store((long long)n, std::memory_order_release);
    const size_t nf = maps.size();
    if (device_pack) {
      bases.resize(n * a.word_length);
      parallel_ranges(n, threads, [&](size_t b, size_t e, unsigned) {
        std::string_view seqs[64], name0, nm, st, ql;
        for (size_t i = b; i < e; i++) {
          for (size_t f = 0; f < nf; f++) {
            maps[f].lines(i, nm, seqs[f], st, ql);
            if (f == 0) name0 = nm;
          }
          gather_bases(name0, seqs, nf, plan, &bases[i * a.word_length]);
        }
      });
    } else {
    words.resize(n * wpr);
    filtered.resize(n);
    if (scoring) scores.resize(n);
    if (positions) { pos_tile.resize(n); pos_x.resize(n); pos_y.resize(n); }
    if (bc_quals) bcq.resize(n * K);
    parallel_ranges(n, threads, [&](size_t b, size_t e, unsigned) {
      std::string_view seqs[64], name0, nm, st, ql;
      for (size_t i = b; i < e; i++) {
        uint64_t qsum = 0;
        for (size_t f = 0; f < nf; f++) {
          maps[f].lines(i, nm, seqs[f], st, ql);
          if (f == 0) name0 = nm;
          if (scoring) qsum += quality_sum(ql.data(), ql.size());
          if (bc_quals && f == 0) put_bc_quals(&bcq[i * K], ql.data(), ql.size());
        }
        if (scoring) scores[i] = clamp_score(qsum);
        if (positions) { const Position ps = parse_position(name0); pos_tile[i] = ps.tile; pos_x[i] = ps.x; pos_y[i] = ps.y; }
        if (a.long_words) {
          filtered[i] = make_word_long(name0, seqs, nf, plan, &words[wpr * i]) ? 1 : 0;
        } else if (wpr == 2) {
          filtered[i] = make_word_wide(name0, seqs, nf, plan, &words[2 * i]) ? 1 : 0;
        } else {
          uint64_t w;
          filtered[i] = make_word(name0, seqs, nf, plan, w) ? 1 : 0;
          words[i] = w;
        }
      }
    });
    }
  } else {
    n_known.store(0, std::memory_order_release);
    MultiReader in(a.files);
    if (!in.ok()) { std::fprintf(stderr, "humid: cannot open %s\n", in.bad_file().c_str()); return 1; }
    std::vector<FastqRecord> recs;
    while (in.next(recs)) {
      uint64_t w[(HUMID_LONG_MAX_NT + 31) / 32];
      bool f = a.long_words ? make_word_long(recs, plan, w) : wpr == 2 ? make_word_wide(recs, plan, w) : make_word(recs, plan, w[0]);
      words.insert(words.end(), w, w + wpr);
      filtered.push_back(f ? 1 : 0);
      if (scoring) {
        uint64_t qsum = 0;
        for (const FastqRecord &r : recs) qsum += quality_sum(r.quality.data(), r.quality.size());
        scores.push_back(clamp_score(qsum));
      }
      if (bc_quals) {
        bcq.resize(bcq.size() + K);
        put_bc_quals(&bcq[bcq.size() - K], recs[0].quality.data(), recs[0].quality.size());
      }
      if (positions) {
        const Position ps = parse_position(recs[0].name);
        pos_tile.push_back(ps.tile); pos_x.push_back(ps.x); pos_y.push_back(ps.y);
      }
    }
  }
  end_message(log, t);
  const uint64_t N = device_pack ? n_records : filtered.size();

  // -P: the canonical words (what -Q compares and --dump-words shows; the run itself takes the words as they are and
  // returns the strands) and, for the dump, the strand of every read
  std::vector<uint64_t> cwords;
  std::vector<uint8_t> strand;
  if (a.paired && (a.best || !a.dump_words.empty() || (a.duplex && !a.dump_consensus.empty()))) {
    cwords = words;
    strand.assign(N ? N : 1, HUMID_STRAND_NONE);
    parallel_ranges(N, threads, [&](size_t b, size_t e, unsigned) {
      for (size_t i = b; i < e; i++)
        if (!filtered[i]) strand[i] = canonical_word(&cwords[i * wpr], wpr, a.word_length) ? HUMID_STRAND_BOTTOM : HUMID_STRAND_TOP;
    });
  }
  if (!a.dump_words.empty()) {   // development aid: host-side parsing can be checked without a GPU
    std::ofstream out(a.dump_words, std::ios::out | std::ios::binary);
    out.write((const char *)&N, 8);
    out.write((const char *)(a.paired ? cwords : words).data(), (std::streamsize)(N * 8 * wpr));
    out.write((const char *)filtered.data(), (std::streamsize)N);
    if (a.paired) out.write((const char *)strand.data(), (std::streamsize)N);   // -P: the canonical words, then one strand byte per read
  }
  if (!a.dump_scores.empty()) {  // ... and the -Q scores: a u64 count, then u32 scores
    std::ofstream out(a.dump_scores, std::ios::out | std::ios::binary);
    out.write((const char *)&N, 8);
    out.write((const char *)scores.data(), (std::streamsize)(N * 4));
  }
  if (!a.dump_bc_quals.empty()) {   // ... and the barcode qualities: a u64 count, then K bytes per read
    std::ofstream out(a.dump_bc_quals, std::ios::out | std::ios::binary);
    out.write((const char *)&N, 8);
    out.write((const char *)bcq.data(), (std::streamsize)(N * K));
  }
  if (!a.dump_positions.empty()) {   // ... and the -O positions: a u64 count, then tile, x and y as three u32 arrays
    std::ofstream out(a.dump_positions, std::ios::out | std::ios::binary);
    out.write((const char *)&N, 8);
    out.write((const char *)pos_tile.data(), (std::streamsize)(N * 4));
    out.write((const char *)pos_x.data(), (std::streamsize)(N * 4));
    out.write((const char *)pos_y.data(), (std::streamsize)(N * 4));
  }
  if (!a.dump_consensus.empty()) {   // ... and what -C hands to the GPU: a u64 count, then per file off u64[n + 1] and the two blobs
    std::ofstream out(a.dump_consensus, std::ios::out | std::ios::binary);
    out.write((const char *)&N, 8);
    for (size_t f = 0; f < maps.size(); f++) {
      std::vector<uint64_t> off;
      std::vector<uint8_t> lb, lq;
      gather_layer(maps[f], N, threads, off, lb, lq);
      out.write((const char *)off.data(), (std::streamsize)((N + 1) * 8));
      out.write((const char *)lb.data(), (std::streamsize)lb.size());
      out.write((const char *)lq.data(), (std::streamsize)lq.size());
    }
    if (a.paired && a.duplex) out.write((const char *)strand.data(), (std::streamsize)N);   // -P -D: then one strand byte per read
  }
  if (dump_only) return 0;

  // -b K: the packed n-nucleotide word splits into the key (its first K nucleotides, one uint64) and the word the
  // run clusters (the remaining n - K, one uint64 up to 32 nucleotides, two beyond): a shift per read
  std::vector<uint64_t> keys;
  const size_t run_nt = a.keyed ? a.word_length - a.barcode : a.word_length;
  if (a.keyed) {
    const size_t out_wpr = run_nt > 32 ? 2 : 1;
    const unsigned rb = 2 * (unsigned)run_nt;              // bits of the remaining word, 2 .. 126
    keys.resize(N);
    std::vector<uint64_t> rest(N * out_wpr);
    parallel_ranges(N, threads, [&](size_t b, size_t e, unsigned) {
      for (size_t i = b; i < e; i++) {
        const unsigned __int128 v = wpr == 2 ? ((unsigned __int128)words[2 * i] << 64) | words[2 * i + 1] : (unsigned __int128)words[i];
        const unsigned __int128 w = v & ((((unsigned __int128)1) << rb) - 1);
        keys[i] = (uint64_t)(v >> rb);
        if (out_wpr == 2) { rest[2 * i] = (uint64_t)(w >> 64); rest[2 * i + 1] = (uint64_t)w; }
        else rest[i] = (uint64_t)w;
      }
    });
    words.swap(rest);
  }

  // ---- the hot path on the GPU ----
  phase("pass 1 done");
  if (ctx_init.th.joinable()) ctx_init.th.join();
  if (!sharded && (ctx_rc != HUMID_OK || !ctx)) {
    std::fprintf(stderr, "humid: %s\n", ctx_err.c_str());
    return 1;
  }
  phase("context ready");
  // results: in the page-locked staging when there is one (pass 2 reads them there), else in vectors
  std::vector<uint32_t> cid_vec;
  std::vector<uint8_t> keep_vec;
  uint32_t *cluster_id = nullptr;
  uint8_t *keep = nullptr;
  const uint64_t *run_words = words.data();
  const uint8_t *run_filt = filtered.data();
  const bool staged = pinned != nullptr && N > 0 && !device_pack && !a.keyed && (uint64_t)n_known.load() == N;
  if (staged) {
    const uint64_t wb = N * 8 * wpr;
    uint8_t *p_words = pinned, *p_filt = pinned + wb;
    cluster_id = (uint32_t *)(pinned + ((wb + N + 15) & ~(uint64_t)15));
    keep = (uint8_t *)(cluster_id + N);
    parallel_ranges(N, threads, [&](size_t b, size_t e, unsigned) {
      memcpy(p_words + b * 8 * wpr, (const uint8_t *)words.data() + b * 8 * wpr, (e - b) * 8 * wpr);
      memcpy(p_filt + b, filtered.data() + b, e - b);
    });
    run_words = (const uint64_t *)p_words;
    run_filt = p_filt;
    phase("words in page-locked staging");
  } else {
    cid_vec.resize(N ? N : 1);
    keep_vec.resize(N ? N : 1);
    cluster_id = cid_vec.data();
    keep = keep_vec.data();
  }
  humid_summary sum;
  std::memset(&sum, 0, sizeof sum);
  if (a.edit) humid_ctx_set_option(ctx, "edit_distance", 1);
  const uint32_t max_inexact = a.max_inexact_given ? (uint32_t)a.max_inexact : (uint32_t)seg_nt.size();
  if (corrected && !discover &&
      (segmented ? humid_whitelist_set_segments(ctx, (uint32_t)seg_nt.size(), seg_nt.data(), seg_n.data(), whitelist.data(), max_inexact)
                 : humid_whitelist_set(ctx, whitelist.data(), whitelist.size(), (uint32_t)a.barcode)) != HUMID_OK) {
    std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx));
    humid_ctx_destroy(ctx);
    return 1;
  }
  humid_cells_summary csum;
  std::memset(&csum, 0, sizeof csum);
  auto cells_line = [&]() {
    log << "  cells: " << csum.cells << " of " << csum.distinct << " barcodes (" << csum.selected << " selected at " << csum.threshold_reads
        << " reads or more, " << csum.merged << " merged away), " << csum.reads_in_cells << " of " << csum.usable
        << " usable reads in cells, largest barcode " << csum.top_reads << " reads, " << csum.invalid_reads << " reads with an invalid barcode\n";
  };
  if (discover) {
    // the whitelist from the data: the barcodes of all usable reads are counted on the device, the cells become the
    // context's whitelist, and what follows is the -w path
    // (--chunk-barcoded: the same counts from a counter fed in chunks, the same selection over them)
    int drc = HUMID_OK;
    if (a.bchunked) {
      drc = humid_cells_begin(ctx, (uint32_t)a.barcode);
      for (uint64_t b = 0; drc == HUMID_OK && b < N; b += a.bchunk_reads)
        drc = humid_cells_add(ctx, keys.data() + b, run_filt + b, std::min<uint64_t>(a.bchunk_reads, N - b));
      if (drc == HUMID_OK) drc = humid_cells_finish(ctx, (uint32_t)a.cells_mode, a.cells_param, (uint32_t)a.cells_ratio, &csum);
      if (drc == HUMID_OK) drc = humid_cells_clear(ctx);
    } else
      drc = humid_whitelist_discover(ctx, keys.data(), run_filt, N, (uint32_t)a.barcode, (uint32_t)a.cells_mode, a.cells_param,
                                     (uint32_t)a.cells_ratio, &csum);
    if (drc != HUMID_OK) {
      std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx));
      humid_ctx_destroy(ctx);
      return 1;
    }
    if (csum.cells == 0) {
      cells_line();
      std::fprintf(stderr, "humid: no cell barcode was found among %llu barcodes of %llu usable reads\n", (unsigned long long)csum.distinct,
                   (unsigned long long)csum.usable);
      humid_ctx_destroy(ctx);
      return 1;
    }
  }
  t = start_message(log, a.edit ? "Calculating neighbours using Levenshtein distance"     // src/humid.cc:142
                                : "Calculating neighbours using Hamming distance");
  const uint32_t method = a.maximum ? HUMID_METHOD_MAXIMUM : HUMID_METHOD_DIRECTIONAL;
  ShardedResult shr;
  int rc;
  uint64_t bc_counts[5] = {0, 0, 0, 0, 0};
  uint64_t bc_multi = 0, bc_rescued = 0;
  uint64_t seg_counts[8 * 4] = {}, inexact_hist[9] = {};
  GroupsTable groups;                                    // --chunk-barcoded -s: fetched before the first map
  if (sharded) {
    // the read set in input-order shards, one rank (thread + context + GPU) per shard: sharded.cpp
    rc = ranks->run(run_words, run_filt, N, (uint32_t)a.word_length, (uint32_t)a.distance, method, a.stats, cluster_id, keep, shr,
                    a.edit);
    sum = shr.sum;
    if (rc == HUMID_OK && getenv("HUMID_TIMING"))
      std::fprintf(stderr, "[humid]   %u ranks, bulk data by %s: set-up %.1f ms, ranks %.1f ms\n", a.gpus,
                   shr.comm.c_str(), shr.ms_init, shr.ms_run);
  } else if (a.chunked) {
    // an accumulated run (include/humid_hip.h): every chunk added with the index of its first record as its base, the
    // list clustered, the histograms fetched at once (the first map ends the record finish published), every chunk mapped
    rc = humid_accum_begin(ctx, (uint32_t)a.word_length);
    for (uint64_t b = 0; rc == HUMID_OK && b < N; b += a.chunk_reads)
      rc = humid_accum_add(ctx, run_words + b * wpr, run_filt + b, std::min<uint64_t>(a.chunk_reads, N - b), b);
    if (rc == HUMID_OK) rc = humid_accum_finish(ctx, (uint32_t)a.distance, method, &sum);
    for (uint32_t which = 0; rc == HUMID_OK && a.stats && which < 3; which++) rc = fetch_hist(ctx, which, shr.hist[which]);
    for (uint64_t b = 0; rc == HUMID_OK && b < N; b += a.chunk_reads)
      rc = humid_accum_map(ctx, run_words + b * wpr, run_filt + b, std::min<uint64_t>(a.chunk_reads, N - b), b, cluster_id + b, keep + b,
                           nullptr);
  } else if (a.bchunked) {
    // a keyed accumulated run (include/humid_hip.h): with --barcode-posterior the reads per whitelist barcode over all
    // chunks first; then every chunk's barcodes corrected (plain, segmented, or by the posterior against that prior; not at
    // all with -b alone) and its entries added with the index of its first record as its base; the list clustered; the
    // histograms and the group table fetched at once (the first map ends the record finish published); every chunk
    // mapped with the corrected keys, which the host keeps.  The status counts are the sums over the chunks.
    const uint64_t cb = a.bchunk_reads;
    std::vector<uint64_t> ckeys(corrected ? (N ? N : 1) : 0);
    std::vector<uint8_t> cfilt(corrected ? (N ? N : 1) : 0), status(corrected ? (size_t)std::min<uint64_t>(cb, N ? N : 1) : 0);
    const uint64_t *akeys = corrected ? ckeys.data() : keys.data();
    const uint8_t *afilt = corrected ? cfilt.data() : run_filt;
    rc = HUMID_OK;
    if (a.posterior) {
      rc = humid_whitelist_prior_begin(ctx);
      for (uint64_t b = 0; rc == HUMID_OK && b < N; b += cb)
        rc = humid_whitelist_prior_add(ctx, keys.data() + b, run_filt + b, std::min<uint64_t>(cb, N - b));
    }
    if (rc == HUMID_OK) rc = humid_accum_begin_keyed(ctx, (uint32_t)run_nt, (uint32_t)a.barcode);
    for (uint64_t b = 0; rc == HUMID_OK && b < N; b += cb) {
      const uint64_t n = std::min<uint64_t>(cb, N - b);
      if (corrected) {
        uint64_t counts[5] = {0, 0, 0, 0, 0};
        if (a.posterior) {
          humid_bc_posterior_summary ps;
          std::memset(&ps, 0, sizeof ps);
          rc = humid_whitelist_correct_posterior_prior(ctx, keys.data() + b, bcq.data() + b * K, run_filt + b, n, (uint32_t)a.min_odds,
                                                       ckeys.data() + b, status.data(), &ps);
          for (int k = 0; k < 5; k++) counts[k] = ps.counts[k];
          bc_multi += ps.multi;
          bc_rescued += ps.rescued;
        } else
          rc = humid_whitelist_correct(ctx, keys.data() + b, run_filt + b, n, ckeys.data() + b, status.data(), counts);
        if (rc == HUMID_OK && segmented) {                   // (answers per correct call)
          uint64_t sc[8 * 4] = {}, ih[9] = {};
          rc = humid_get_barcode_segments(ctx, sc, ih);
          for (int k = 0; k < 8 * 4; k++) seg_counts[k] += sc[k];
          for (int k = 0; k < 9; k++) inexact_hist[k] += ih[k];
        }
        if (rc != HUMID_OK) break;
        for (int k = 0; k < 5; k++) bc_counts[k] += counts[k];
        for (uint64_t i = 0; i < n; i++) cfilt[b + i] = (uint8_t)(run_filt[b + i] | (status[i] >= HUMID_BC_AMBIGUOUS ? 1 : 0));
      }
      rc = humid_accum_add_keyed(ctx, run_words + b, akeys + b, afilt + b, n, b);
    }
    if (rc == HUMID_OK) rc = humid_accum_finish(ctx, (uint32_t)a.distance, method, &sum);
    for (uint32_t which = 0; rc == HUMID_OK && a.stats && which < 3; which++) rc = fetch_hist(ctx, which, shr.hist[which]);
    if (rc == HUMID_OK && a.stats && fetch_groups(ctx, groups) != 1) rc = HUMID_E_STATE;
    for (uint64_t b = 0; rc == HUMID_OK && b < N; b += cb)
      rc = humid_accum_map_keyed(ctx, run_words + b, akeys + b, afilt + b, std::min<uint64_t>(cb, N - b), b, cluster_id + b, keep + b,
                                 nullptr);
  } else if (a.posterior)
    rc = humid_dedup_run_keyed_posterior(ctx, run_words, keys.data(), bcq.data(), run_filt, N, (uint32_t)run_nt, (uint32_t)a.distance,
                                         method, (uint32_t)a.min_odds, cluster_id, keep, &sum);
  else if (corrected)
    rc = humid_dedup_run_keyed_corrected(ctx, run_words, keys.data(), run_filt, N, (uint32_t)run_nt, (uint32_t)a.distance,
                                         method, cluster_id, keep, &sum);
  else if (a.paired)
    rc = humid_dedup_run_paired(ctx, run_words, run_filt, N, (uint32_t)a.word_length, (uint32_t)a.distance, method, cluster_id,
                                keep, &sum);
  else if (a.keyed)
    rc = humid_dedup_run_keyed(ctx, run_words, keys.data(), run_filt, N, (uint32_t)run_nt, (uint32_t)a.distance, method,
                               cluster_id, keep, &sum);
  else if (a.long_words)
    rc = humid_dedup_run_long(ctx, run_words, run_filt, N, (uint32_t)a.word_length, (uint32_t)a.distance, method, cluster_id, keep,
                              &sum);
  else
  rc = device_pack
               ? humid_dedup_run_bases(ctx, bases.data(), N, (uint32_t)a.word_length, (uint32_t)a.distance, method,
                                       cluster_id, keep, &sum)
               : humid_dedup_run(ctx, run_words, run_filt, N, (uint32_t)a.word_length,
                                 (uint32_t)a.distance, method, cluster_id, keep, &sum);
  if (rc != HUMID_OK) {
    log << "failed.\n";
    std::fprintf(stderr, "humid: %s\n", sharded ? shr.error.c_str() : humid_last_error(ctx));
    humid_ctx_destroy(ctx);
    return 1;
  }
  // (--chunk-barcoded has summed these over its chunks)
  if (rc == HUMID_OK && corrected && !a.bchunked) rc = humid_get_barcode_status(ctx, nullptr, 0, bc_counts);
  if (rc == HUMID_OK && a.posterior && !a.bchunked) rc = humid_get_barcode_posterior(ctx, &bc_multi, &bc_rescued);
  if (rc == HUMID_OK && segmented && !a.bchunked) rc = humid_get_barcode_segments(ctx, seg_counts, inexact_hist);
  humid_strand_summary ssum;
  std::memset(&ssum, 0, sizeof ssum);
  if (rc == HUMID_OK && a.paired) {
    strand.assign(N ? N : 1, HUMID_STRAND_NONE);
    rc = humid_get_strands(ctx, strand.data(), N, nullptr, nullptr, &ssum);
  }
  if (rc != HUMID_OK) {
    log << "failed.\n";
    std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx));
    humid_ctx_destroy(ctx);
    return 1;
  }
  end_message(log, t);
  uint64_t n_changed = 0;
  if (a.best) {
    // every cluster keeps its best record among those of its most abundant word; keep is rewritten in place and
    // pass 2 follows it (the ids do not move: the annotated files and the statistics are those of the run)
    if (humid_select_best(ctx, a.paired ? cwords.data() : run_words, cluster_id, keep, scores.data(), N, (uint32_t)run_nt, HUMID_BEST_LEAF, keep, nullptr,
                          &n_changed) != HUMID_OK) {
      log << "failed.\n";
      std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx));
      humid_ctx_destroy(ctx);
      return 1;
    }
  }
  if (discover) cells_line();
  if (corrected)
    log << "  barcodes: " << bc_counts[HUMID_BC_EXACT] << " exact, " << bc_counts[HUMID_BC_CORRECTED] << " corrected, "
        << bc_counts[HUMID_BC_AMBIGUOUS] << " ambiguous, " << bc_counts[HUMID_BC_UNMATCHED] << " unmatched\n";
  if (segmented) {
    log << "  barcode segments (exact/corrected/ambiguous/unmatched):";
    for (size_t g = 0; g < seg_nt.size(); g++)
      log << ' ' << seg_counts[4 * g] << '/' << seg_counts[4 * g + 1] << '/' << seg_counts[4 * g + 2] << '/' << seg_counts[4 * g + 3];
    log << "; reads by segments not exact (at most " << max_inexact << "):";
    for (size_t m = 0; m <= seg_nt.size(); m++) log << ' ' << inexact_hist[m];
    log << '\n';
  }
  if (a.posterior)
    log << "  barcode posterior: " << bc_multi << " reads with several candidates, " << bc_rescued << " of them corrected (odds >= "
        << a.min_odds << ")\n";
  if (a.paired)
    log << "  strands: " << ssum.n_clusters << " clusters, " << ssum.duplex << " duplex, " << ssum.top_only << " top only, "
        << ssum.bottom_only << " bottom only; " << ssum.top_reads << " top reads, " << ssum.bottom_reads << " bottom reads\n";
  if (a.best) log << "  quality: " << n_changed << " clusters keep another record\n";
  // -O: after -Q, so that the origin of a group follows the final keep
  humid_optical_summary osum;
  std::memset(&osum, 0, sizeof osum);
  uint64_t n_positioned = 0;
  if (a.optical) {
    std::vector<uint8_t> is_optical(N ? N : 1);
    if (humid_optical_duplicates(ctx, cluster_id, keep, pos_tile.data(), pos_x.data(), pos_y.data(), N, sum.clusters, a.optical_distance,
                                 is_optical.data(), nullptr, nullptr, &osum) != HUMID_OK) {
      log << "failed.\n";
      std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx));
      humid_ctx_destroy(ctx);
      return 1;
    }
    for (uint64_t i = 0; i < N; i++) n_positioned += pos_tile[i] != HUMID_NO_TILE;
    log << "  optical: " << osum.optical << " of " << osum.duplicates << " duplicates in " << osum.groups << " groups\n";
    log << "  positions: " << n_positioned << " of " << N << " records\n";
  }
  // -C: one consensus pass per input file, one after the other (a file's blobs are freed before the next is gathered);
  // what pass 2 needs stays on the host: per file the offsets and the two consensus blobs, in cluster-id order
  std::vector<std::vector<uint64_t>> cons_off(cons_out ? maps.size() : 0);
  std::vector<std::vector<uint8_t>> cons_b(cons_off.size()), cons_q(cons_off.size());
  if (a.consensus) {
    uint64_t changed = 0, disagree = 0, multi = 0;
    for (size_t f = 0; f < maps.size(); f++) {
      humid_consensus_summary cs;
      std::memset(&cs, 0, sizeof cs);
      int crc;
      {
        std::vector<uint64_t> off;
        std::vector<uint8_t> lb, lq;
        gather_layer(maps[f], N, threads, off, lb, lq);
        crc = humid_consensus(ctx, lb.data(), lq.data(), off.data(), off[N], cluster_id, keep, N, sum.clusters, a.consensus_min_q, 93, &cs);
      }
      if (crc == HUMID_OK) {
        cons_off[f].resize(cs.n_clusters + 1);
        cons_b[f].resize(cs.total_bytes ? cs.total_bytes : 1);
        cons_q[f].resize(cs.total_bytes ? cs.total_bytes : 1);
        crc = humid_get_consensus(ctx, cs.total_bytes, cons_off[f].data(), cons_b[f].data(), cons_q[f].data(), nullptr, nullptr);
      }
      if (crc == HUMID_OK && cs.n_clusters != sum.clusters && N) crc = HUMID_E_STATE;   // (cannot happen: C was passed in)
      if (crc != HUMID_OK) {
        log << "failed.\n";
        std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx));
        humid_ctx_destroy(ctx);
        return 1;
      }
      changed += cs.bases_changed;
      disagree += cs.errors;
      multi = cs.multi_read;
    }
    // (clusters and multi-read clusters are those of the run; bases changed and disagreeing votes add up over the files)
    log << "  consensus: " << sum.clusters << " clusters, " << multi << " multi-read, " << changed << " bases changed, "
        << disagree << " disagreeing votes\n";
  }
  // -D: both files' blobs are resident at once; output layer f takes file f as the same layer and the other file as
  // the other layer.  The results come back through humid_get_consensus, so pass 2 is that of -C.
  humid_duplex_summary dsum[2];
  std::memset(dsum, 0, sizeof dsum);
  if (a.duplex) {
    std::vector<uint64_t> off[2];
    std::vector<uint8_t> lb[2], lq[2];
    for (size_t f = 0; f < 2; f++) gather_layer(maps[f], N, threads, off[f], lb[f], lq[f]);
    for (size_t f = 0; f < 2; f++) {
      const size_t g = 1 - f;
      humid_duplex_summary &ds = dsum[f];
      int crc = humid_duplex_consensus(ctx, lb[f].data(), lq[f].data(), off[f].data(), off[f][N], lb[g].data(), lq[g].data(), off[g].data(),
                                       off[g][N], cluster_id, keep, strand.data(), N, sum.clusters, a.consensus_min_q, a.duplex_strand_cap,
                                       93, &ds);
      if (crc == HUMID_OK) {
        cons_off[f].resize(ds.n_clusters + 1);
        cons_b[f].resize(ds.total_bytes ? ds.total_bytes : 1);
        cons_q[f].resize(ds.total_bytes ? ds.total_bytes : 1);
        crc = humid_get_consensus(ctx, ds.total_bytes, cons_off[f].data(), cons_b[f].data(), cons_q[f].data(), nullptr, nullptr);
      }
      if (crc == HUMID_OK && ds.n_clusters != sum.clusters && N) crc = HUMID_E_STATE;   // (cannot happen: C was passed in)
      if (crc != HUMID_OK) {
        log << "failed.\n";
        std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx));
        humid_ctx_destroy(ctx);
        return 1;
      }
    }
    // (clusters are those of the run; the columns add up over the two files)
    log << "  duplex consensus: " << sum.clusters << " clusters, " << dsum[0].duplex_clusters << " duplex, "
        << dsum[0].both_called + dsum[1].both_called << " columns called by both strands, " << dsum[0].agree + dsum[1].agree << " agree, "
        << dsum[0].disagree + dsum[1].disagree << " disagree, " << dsum[0].masked + dsum[1].masked << " masked, "
        << dsum[0].bases_changed + dsum[1].bases_changed << " bases changed\n";
  }
  // the kept record i of file f, copied to dst, takes the consensus of its cluster on its sequence and quality lines
  auto put_consensus = [&](size_t f, size_t i, char *dst) {
    std::string_view nm, sq, st, ql;
    maps[f].lines(i, nm, sq, st, ql);
    const char *r0 = maps[f].raw(i).data();
    const uint64_t o = cons_off[f][cluster_id[i] - 1], len = cons_off[f][cluster_id[i]] - o;
    if (len) {
      memcpy(dst + (sq.data() - r0), &cons_b[f][o], (size_t)len);
      memcpy(dst + (ql.data() - r0), &cons_q[f][o], (size_t)len);
    }
  };
  // what -a appends to the header of record i: ':' + cluster id (src/humid.cc:281) and, with -P, "/A" for a read taken
  // as given, "/B" for one taken exchanged (nothing for an unusable read: ":0")
  auto tag_size = [&](size_t i) {
    size_t d = 1;
    for (uint32_t v = cluster_id[i]; v >= 10; v /= 10) d++;
    return 1 + d + ((a.paired && strand[i] != HUMID_STRAND_NONE) ? (size_t)2 : (size_t)0);
  };
  auto put_tag = [&](size_t i, char *q) {
    *q++ = ':';
    char dig[10];
    unsigned nd = 0;
    uint32_t v = cluster_id[i];
    do { dig[nd++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (nd) *q++ = dig[--nd];
    if (a.paired && strand[i] != HUMID_STRAND_NONE) { *q++ = '/'; *q++ = strand[i] == HUMID_STRAND_BOTTOM ? 'B' : 'A'; }
    return q;
  };
  phase("device path done");
  if (getenv("HUMID_TIMING"))
    std::fprintf(stderr, "[humid]   of which on the device: upload%s %.1f ms, hot path %.2f ms, download %.1f ms\n",
                 device_pack ? " + packing" : "", sum.ms_h2d, sum.ms_total, sum.ms_d2h);
  t = start_message(log, a.maximum ? "Calculating maximum clusters" : "Calculating directional clusters");
  end_message(log, t);
  std::vector<uint64_t>().swap(words);
  std::vector<uint64_t>().swap(cwords);
  std::vector<uint64_t>().swap(keys);
  std::vector<uint32_t>().swap(scores);
  std::vector<uint32_t>().swap(pos_tile);
  std::vector<uint32_t>().swap(pos_x);
  std::vector<uint32_t>().swap(pos_y);
  std::vector<uint8_t>().swap(bases);

  make_dirs(a.dir_name);

  // ---- pass 2: writeFiltered (src/humid.cc:203-241) / writeAnnotated (:251-292) ----
  if (a.filter || a.annotate) {
    time_t tf = 0, ta = 0;
    if (a.filter) tf = start_message(log, "Writing filtered results");
    std::vector<FastqWriter *> dedup, annot;
    for (const std::string &f : a.files) {
      // fast path: .gz outputs are written as gzip members compressed on all cores
      if (a.filter) dedup.push_back(new FastqWriter(make_file_name(f, a.dir_name, "dedup"), fast));
      if (a.annotate) annot.push_back(new FastqWriter(make_file_name(f, a.dir_name, "annotated"), fast));
    }
    bool ok = true;
    for (FastqWriter *w : dedup) ok = ok && w->ok();
    for (FastqWriter *w : annot) ok = ok && w->ok();
    if (!ok) { std::fprintf(stderr, "humid: cannot create output files in %s\n", a.dir_name.c_str()); return 1; }
    // plain outputs of the fast path go through a shared mapping (write_mapped); what it cannot take
    // (gzip outputs, files that cannot be preallocated) goes through the batch loop below
    std::vector<char> done_dedup(a.files.size(), 0), done_annot(a.files.size(), 0);
    bool mapped_failed = false;
    if (fast && getenv("HUMID_NO_MAPPED_WRITE") == nullptr) {
      // the files of a pair are written side by side (page-cache filling scales per file), each with
      // its share of the workers
      const unsigned per_file = threads / (unsigned)maps.size() ? threads / (unsigned)maps.size() : 1;
      std::vector<char> failed_f(maps.size(), 0);
      std::vector<std::thread> file_workers;
      for (size_t f = 0; f < maps.size(); f++) file_workers.emplace_back([&, f] {
        const unsigned threads = per_file;               // (shadows: this file's share)
        bool mapped_failed = false;
        if (a.filter && !dedup[f]->gz_members()) {
          const std::string path = make_file_name(a.files[f], a.dir_name, "dedup");
          const int r = write_mapped(path, N, threads,
              [&](size_t i) { return keep[i] ? maps[f].raw(i).size() : (size_t)0; },
              [&](size_t i, char *q) {
                if (!keep[i]) return q;
                const std::string_view rr = maps[f].raw(i);
                memcpy(q, rr.data(), rr.size());
                if (cons_out) put_consensus(f, i, q);
                return q + rr.size();
              });
          if (r > 0) done_dedup[f] = 1;
          if (r < 0) mapped_failed = true;
        }
        if (a.annotate && !annot[f]->gz_members()) {
          // annotated record = header + ':' + cluster id + the rest of the record verbatim (src/humid.cc:281)
          const std::string path = make_file_name(a.files[f], a.dir_name, "annotated");
          const int r = write_mapped(path, N, threads,
              [&](size_t i) { return maps[f].raw(i).size() + tag_size(i); },
              [&](size_t i, char *q) {
                const std::string_view rr = maps[f].raw(i);
                const char *nl = (const char *)memchr(rr.data(), '\n', rr.size());
                const size_t hl = nl ? (size_t)(nl - rr.data()) : rr.size();
                memcpy(q, rr.data(), hl);
                q = put_tag(i, q + hl);
                memcpy(q, rr.data() + hl, rr.size() - hl);
                return q + (rr.size() - hl);
              });
          if (r > 0) done_annot[f] = 1;
          if (r < 0) mapped_failed = true;
        }
        failed_f[f] = mapped_failed ? 1 : 0;
      });
      for (auto &th : file_workers) th.join();
      for (char x : failed_f) mapped_failed = mapped_failed || x;
    }
    if (fast) {
      // records come straight from the mappings; batches are formatted on all cores and written
      // in order
      const size_t nf = maps.size();
      const size_t batch = 1u << 20;
      std::vector<std::string> bufs(threads), zbufs(threads);
      for (size_t b0 = 0; b0 < N; b0 += batch) {
        const size_t b1 = b0 + batch < N ? b0 + batch : N;
        for (size_t f = 0; f < nf; f++) {
          for (int what = 0; what < 2; what++) {           // 0 = dedup, 1 = annotated
            if ((what == 0 && !a.filter) || (what == 1 && !a.annotate)) continue;
            if ((what == 0 && done_dedup[f]) || (what == 1 && done_annot[f])) continue;   // written through the mapping
            FastqWriter *wr = what == 0 ? dedup[f] : annot[f];
            const bool zip = wr->gz_members();
            parallel_ranges(b1 - b0, threads, [&](size_t rb, size_t re, unsigned w) {
              std::string &o = bufs[w];
              o.clear();
              if (what == 0) {
                for (size_t i = b0 + rb; i < b0 + re; i++)
                  if (keep[i]) {
                    std::string_view r = maps[f].raw(i);
                    o.append(r.data(), r.size());
                    if (cons_out) put_consensus(f, i, &o[o.size() - r.size()]);
                  }
              } else if (re > rb) {
                // annotated record = header + ':' + cluster id + the rest of the record verbatim
                // (src/humid.cc:281); written with pointer arithmetic into a buffer sized up front
                const size_t first = b0 + rb, last = b0 + re;
                const size_t in_bytes = (size_t)(maps[f].rec_off[last] - maps[f].rec_off[first]);
                o.resize(in_bytes + 13 * (last - first));
                char *q = &o[0];
                for (size_t i = first; i < last; i++) {
                  const std::string_view r = maps[f].raw(i);
                  const char *nl = (const char *)memchr(r.data(), '\n', r.size());
                  const size_t hl = nl ? (size_t)(nl - r.data()) : r.size();
                  memcpy(q, r.data(), hl);
                  q = put_tag(i, q + hl);
                  memcpy(q, r.data() + hl, r.size() - hl);
                  q += r.size() - hl;
                }
                o.resize((size_t)(q - o.data()));
              }
              if (zip) {
                zbufs[w].clear();
                if (!o.empty()) FastqWriter::compress_member(o.data(), o.size(), zbufs[w]);
              }
            });
            const unsigned used = (threads <= 1 || b1 - b0 < 4096) ? 1 : threads;
            wr->write_parts(zip ? zbufs : bufs, used);       // every part at its final offset, in parallel
          }
        }
      }
    } else {
    MultiReader in(a.files);
    std::vector<FastqRecord> recs;
    std::string s;
    uint64_t i = 0;
    while (i < N && in.next(recs)) {
      if (a.filter && keep[i]) {
        for (size_t f = 0; f < recs.size(); f++) {
          s.clear();
          recs[f].append_to(s);
          dedup[f]->write(s.data(), s.size());
        }
      }
      if (a.annotate) {
        char tagbuf[16];
        const std::string tag(tagbuf, (size_t)(put_tag(i, tagbuf) - tagbuf));
        for (size_t f = 0; f < recs.size(); f++) {
          recs[f].name += tag;
          s.clear();
          recs[f].append_to(s);
          annot[f]->write(s.data(), s.size());
        }
      }
      i++;
    }
    }
    // a short or failed write (disk full, I/O error) must not end in exit code 0
    bool wrote_ok = !mapped_failed;
    // (a FastqWriter whose file went through the mapping wrote nothing: it must not truncate the file)
    for (size_t f = 0; f < dedup.size(); f++) { if (!done_dedup[f]) wrote_ok = dedup[f]->close() && wrote_ok; delete dedup[f]; }
    for (size_t f = 0; f < annot.size(); f++) { if (!done_annot[f]) wrote_ok = annot[f]->close() && wrote_ok; delete annot[f]; }
    if (!wrote_ok) {
      log << "failed.\n";
      std::fprintf(stderr, "humid: writing the output FastQ files in %s failed (disk full or I/O error): "
                           "the outputs are incomplete\n", a.dir_name.c_str());
      humid_ctx_destroy(ctx);
      return 1;
    }
    if (a.filter) end_message(log, tf);
    if (a.annotate) { ta = start_message(log, "Writing annotated results"); end_message(log, ta); }
  }

  if (fast && getenv("HUMID_SLOW_EXIT") == nullptr)
    for (auto &m : maps) m.drop_pages(threads);          // the inputs are not read again
  phase("pass 2 done");
  // ---- statistics (src/humid.cc:301-357, src/cluster.cc:89-95) ----
  if (a.stats) {
    t = start_message(log, "Calculating count and neighbour stats");
    const char *names[3] = {"/counts.dat", "/neigh.dat", "/clusters.dat"};
    int ok = 1;
    for (uint32_t which = 0; which < 3 && ok == 1; which++) {
      if (!sharded && !a.chunked && !a.bchunked) { ok = write_hist(ctx, which, a.dir_name + names[which]); continue; }
      std::ofstream out(a.dir_name + names[which], std::ios::out | std::ios::binary);   // gathered by the ranks, or fetched after the finish of an accumulated run
      for (auto &kv : shr.hist[which]) out << kv.first << ' ' << kv.second << '\n';
      out.close();
      if (out.fail()) ok = -1;
    }
    if (ok == 1 && a.keyed && !a.bchunked) ok = fetch_groups(ctx, groups);   // (-b is never sharded)
    if (ok == 1 && a.keyed) ok = write_groups(groups, a.barcode, a.dir_name + "/groups.dat");
    if (ok == 1 && corrected) {
      std::ofstream out(a.dir_name + "/barcodes.dat", std::ios::out | std::ios::binary);
      out << "exact: " << bc_counts[HUMID_BC_EXACT] << '\n';
      out << "corrected: " << bc_counts[HUMID_BC_CORRECTED] << '\n';
      out << "ambiguous: " << bc_counts[HUMID_BC_AMBIGUOUS] << '\n';
      out << "unmatched: " << bc_counts[HUMID_BC_UNMATCHED] << '\n';
      if (a.posterior) {
        out << "multi: " << bc_multi << '\n';
        out << "rescued: " << bc_rescued << '\n';
      }
      if (segmented) {
        const char *cls[4] = {"exact", "corrected", "ambiguous", "unmatched"};
        for (size_t g = 0; g < seg_nt.size(); g++)
          for (int k = 0; k < 4; k++) out << "segment" << g << '.' << cls[k] << ": " << seg_counts[4 * g + k] << '\n';
        for (size_t m = 0; m <= seg_nt.size(); m++) out << "inexact" << m << ": " << inexact_hist[m] << '\n';
      }
      out.close();
      if (out.fail()) ok = -1;
    }
    if (ok == 1 && discover) ok = write_cells(ctx, a.barcode, a.dir_name + "/cells.dat", a.dir_name + "/barcode_rank.dat");
    if (ok == 1 && a.paired) {
      std::ofstream out(a.dir_name + "/strands.dat", std::ios::out | std::ios::binary);
      out << "clusters: " << ssum.n_clusters << '\n';
      out << "duplex: " << ssum.duplex << '\n';
      out << "top_only: " << ssum.top_only << '\n';
      out << "bottom_only: " << ssum.bottom_only << '\n';
      out << "top_reads: " << ssum.top_reads << '\n';
      out << "bottom_reads: " << ssum.bottom_reads << '\n';
      out.close();
      if (out.fail()) ok = -1;
    }
    if (ok == 1 && a.duplex) {                               // the summary of each file's call: file<k>.<field> value
      std::ofstream out(a.dir_name + "/duplex.dat", std::ios::out | std::ios::binary);
      for (size_t f = 0; f < 2; f++) {
        const humid_duplex_summary &d = dsum[f];
        const char *names[11] = {"n_clusters", "total_bytes", "multi_read", "bases_changed", "votes", "errors", "duplex_clusters",
                                 "both_called", "agree", "disagree", "masked"};
        const uint64_t vals[11] = {d.n_clusters, d.total_bytes, d.multi_read, d.bases_changed, d.votes, d.errors, d.duplex_clusters,
                                   d.both_called, d.agree, d.disagree, d.masked};
        for (int k = 0; k < 11; k++) out << "file" << f + 1 << '.' << names[k] << ' ' << vals[k] << '\n';
      }
      out.close();
      if (out.fail()) ok = -1;
    }
    if (ok == 1 && a.optical) {
      std::ofstream out(a.dir_name + "/optical.dat", std::ios::out | std::ios::binary);
      out << "members " << osum.members << '\n';
      out << "duplicates " << osum.duplicates << '\n';
      out << "optical " << osum.optical << '\n';
      out << "pcr " << osum.duplicates - osum.optical << '\n';
      out << "groups " << osum.groups << '\n';
      out << "largest_group " << osum.largest_group << '\n';
      out << "records_without_position " << N - n_positioned << '\n';
      out.close();
      if (out.fail()) ok = -1;
    }
    end_message(log, t);
    if (ok == 0) { std::fprintf(stderr, "humid: %s\n", humid_last_error(ctx)); humid_ctx_destroy(ctx); return 1; }
    std::ofstream out(a.dir_name + "/stats.dat", std::ios::out | std::ios::binary);
    out << "total: " << sum.total << '\n';
    out << "usable: " << sum.usable << '\n';
    out << "unique: " << sum.unique << '\n';
    out << "clusters: " << sum.clusters << '\n';
    out.close();
    if (ok < 0 || out.fail()) {
      std::fprintf(stderr, "humid: writing the statistics files in %s failed\n", a.dir_name.c_str());
      humid_ctx_destroy(ctx);
      return 1;
    }
  }
  log.close();
  if (log.fail()) std::fprintf(stderr, "humid: writing the log %s failed\n", a.log_name.c_str());
  phase("outputs closed");
  if (getenv("HUMID_SLOW_EXIT")) humid_host_free(pinned);     // (the quick exit below leaves it to the kernel)
  humid_ctx_destroy(ctx);
  phase("context destroyed");
  // every output is closed: leave without the static destructors of the HIP runtime and without
  // unmapping the inputs page by page (HUMID_SLOW_EXIT=1 keeps the ordinary exit)
  if (getenv("HUMID_TIMING")) {                          // against the caller's clock: start-up and tear-down outside main()
    timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    std::fprintf(stderr, "[humid] leaving main() at %.6f (epoch s)\n", (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec);
  }
  if (getenv("HUMID_SLOW_EXIT") == nullptr) {
    std::fflush(nullptr);
    _exit(0);
  }
  return 0;
}
