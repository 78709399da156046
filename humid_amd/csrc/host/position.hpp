// position.hpp -- the flowcell position of a record, from its Illumina name, for `humid -O`
// (humid_optical_duplicates, include/humid_hip.h).
//
// The name is the header line up to the first space (with or without the leading '@'), split on ':'.  With at least
// seven fields, field 4 is the lane, 5 the tile, 6 x and 7 y:  @inst:run:flowcell:lane:tile:x:y.  Lane, tile and x
// are runs of decimal digits that fill their field; y is the run of digits its field starts with, so both
// ...:4678:1110_AGTA and ...:4678:1110:AGTA parse.  The tile key is lane << 24 | tile.  A record has NO position
// (tile = POSITION_NONE = HUMID_NO_TILE, x = y = 0) when the name has fewer than seven fields, one of the four is
// empty or holds anything but digits, the lane is >= 255, the tile >= 2^24, or x or y does not fit 32 bits.
// The flowcell field is not looked at: a file is taken to be one flowcell.
#pragma once
#include <cstdint>
#include <string_view>

namespace humid_host {

constexpr uint32_t POSITION_NONE = 0xffffffffu;

struct Position {
  uint32_t tile = POSITION_NONE, x = 0, y = 0;
};

// the digits s starts with -> value; false when there are none or the value exceeds limit.  *used = digits read.
inline bool position_digits(std::string_view s, uint64_t limit, uint64_t &value, size_t *used) {
  uint64_t v = 0;
  size_t i = 0;
  for (; i < s.size() && s[i] >= '0' && s[i] <= '9'; i++) {
    v = v * 10 + (uint64_t)(s[i] - '0');
    if (v > limit) return false;                      // (limit < 2^32: v never wraps)
  }
  if (i == 0) return false;
  value = v;
  *used = i;
  return true;
}

inline Position parse_position(std::string_view header) {
  const size_t sp = header.find(' ');
  const std::string_view name = header.substr(0, sp);  // (npos: the whole line)
  std::string_view f[4];                               // fields 4 .. 7
  size_t at = 0;
  for (int k = 1; k <= 7; k++) {
    if (at > name.size()) return Position{};           // fewer than seven fields
    size_t colon = name.find(':', at);
    if (colon == std::string_view::npos) colon = name.size();
    if (k >= 4) f[k - 4] = name.substr(at, colon - at);
    at = colon + 1;
  }
  uint64_t lane, tile, x, y;
  size_t n;
  if (!position_digits(f[0], 254, lane, &n) || n != f[0].size()) return Position{};
  if (!position_digits(f[1], (1u << 24) - 1, tile, &n) || n != f[1].size()) return Position{};
  if (!position_digits(f[2], 0xffffffffull, x, &n) || n != f[2].size()) return Position{};
  if (!position_digits(f[3], 0xffffffffull, y, &n)) return Position{};
  return Position{(uint32_t)(lane << 24 | tile), (uint32_t)x, (uint32_t)y};
}

}  // namespace humid_host
