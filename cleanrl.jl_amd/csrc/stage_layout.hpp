// stage_layout.hpp — where the sections of one staged call sit in a scratch buffer. Plain C++, no HIP header: stage.hpp puts the transfers on top,
// and tests/test_stage_cpu.py compiles this file alone on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace crl {

constexpr size_t STAGE_ALIGN = 16;   // every section starts on a multiple of this (the widest vector load), whatever the sections before it hold
constexpr int STAGE_MAX_SECTIONS = 8;

// Sections are declared in order as (element size, count); each gets the next 16-byte-aligned offset, `total` is the end of the last one. A section
// list whose bytes do not fit a size_t (or that has more than STAGE_MAX_SECTIONS entries) raises `bad` instead of wrapping, and gets no bytes.
struct StageLayout {
  size_t off[STAGE_MAX_SECTIONS] = {}, bytes[STAGE_MAX_SECTIONS] = {};
  int n = 0;
  size_t total = 0;
  bool bad = false;

  int add(size_t elem, size_t count) {
    if (n == STAGE_MAX_SECTIONS) { bad = true; return 0; }
    const int i = n++;
    if (total > SIZE_MAX - (STAGE_ALIGN - 1)) { bad = true; return i; }
    const size_t at = (total + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1);
    off[i] = at;
    if (count != 0 && elem > (SIZE_MAX - at) / count) { bad = true; return i; }
    bytes[i] = elem * count;
    total = at + bytes[i];
    return i;
  }
};

}  // namespace crl
