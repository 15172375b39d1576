"""CPU-side check of the section layout every staged host call uses (csrc/stage_layout.hpp): a stand-alone C++ program that includes only that
HIP-free header, built with the address and undefined-behaviour sanitizers and run as an ordinary executable.

The expected totals of the three replayed calls are worked out by hand below. `was` is what the hand-written offset arithmetic of the entry point
computed before the calls moved onto the helper (packed sections, only the observations rounded up to 16 bytes); the helper starts EVERY section on
a 16-byte boundary, so its total is `was` plus padding: never less, and less than 16 bytes per section more — equal where every section is already
a multiple of 16 bytes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cleanrl.jl_amd", "csrc")

PROGRAM = r"""
#include "stage_layout.hpp"

#include <cstdio>
#include <cstdlib>

using crl::StageLayout;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

struct Sec { size_t elem, count; };

// the properties every layout has: aligned offsets, sections in order without overlap, total = the last section's end
static StageLayout build(const Sec* secs, int n) {
  StageLayout l;
  for (int i = 0; i < n; ++i) CHECK(l.add(secs[i].elem, secs[i].count) == i);
  CHECK(!l.bad && l.n == n);
  size_t end = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(l.off[i] % 16 == 0);
    CHECK(l.off[i] >= end);                       // no overlap with any earlier section
    CHECK(l.off[i] - end < 16);                   // and nothing but padding between them
    CHECK(l.bytes[i] == secs[i].elem * secs[i].count);
    end = l.off[i] + l.bytes[i];
  }
  CHECK(l.total == end);
  return l;
}

// one replayed call: the helper's total is the hand-computed one; against the packed arithmetic it replaced it only adds padding
static void replay(const Sec* secs, int n, size_t want, size_t was) {
  const StageLayout l = build(secs, n);
  CHECK(l.total == want);
  CHECK(l.total >= was && l.total - was < 16 * (size_t)n);
}

int main() {
  static_assert(crl::STAGE_ALIGN == 16, "sections start on 16-byte boundaries");

  // element sizes 1, 4 and 8 mixed, odd counts
  {
    const Sec s[] = {{1, 3}, {8, 5}, {4, 7}, {1, 17}, {8, 1}};
    const StageLayout l = build(s, 5);
    CHECK(l.off[0] == 0 && l.off[1] == 16 && l.off[2] == 64 && l.off[3] == 96 && l.off[4] == 128 && l.total == 136);
  }
  // a zero-count section has size 0 and its neighbours sit where they sit without it
  {
    const Sec with[] = {{4, 5}, {8, 0}, {4, 3}}, without[] = {{4, 5}, {4, 3}};
    const StageLayout a = build(with, 3), b = build(without, 2);
    CHECK(a.bytes[1] == 0);
    CHECK(a.off[0] == b.off[0] && a.off[2] == b.off[1] && a.total == b.total);
    const Sec lead[] = {{4, 0}, {8, 2}}, trail[] = {{8, 2}, {1, 0}};
    CHECK(build(lead, 2).off[1] == 0 && build(lead, 2).total == 16);
    CHECK(build(trail, 2).total == 16);
  }
  // sizes that do not fit a size_t are an error, never a wrapped total
  {
    StageLayout l;
    l.add(8, SIZE_MAX / 8 + 1);                   // 8 * count wraps to 0
    CHECK(l.bad);
    StageLayout m;
    m.add(4, 4);
    m.add(8, SIZE_MAX / 8);                       // fits alone, not behind 16 bytes
    CHECK(m.bad);
    StageLayout k;
    k.add(8, SIZE_MAX / 8);                       // SIZE_MAX - 7 bytes: fits
    CHECK(!k.bad && k.total == SIZE_MAX - 7);
    k.add(1, 1);                                  // no aligned offset is left behind it
    CHECK(k.bad);
    StageLayout few;
    for (int i = 0; i < crl::STAGE_MAX_SECTIONS; ++i) few.add(4, 1);
    CHECK(!few.bad);
    few.add(4, 1);                                // one section too many
    CHECK(few.bad && few.n == crl::STAGE_MAX_SECTIONS);
  }

  // crl_policy_act at obs_dim 4: obs f32 [4n] | u f64 [n] | action i32 [n] | logprob f32 [n] | value f32 [n].
  // was: round16(16n) + 8n + 4n + 4n + 4n
  {
    const Sec n1[] = {{4, 4}, {8, 1}, {4, 1}, {4, 1}, {4, 1}};      // 0..16 | 16..24 | 32..36 | 48..52 | 64..68
    replay(n1, 5, 68, 36);
    const Sec n3[] = {{4, 12}, {8, 3}, {4, 3}, {4, 3}, {4, 3}};     // 0..48 | 48..72 | 80..92 | 96..108 | 112..124
    replay(n3, 5, 124, 108);
  }
  // crl_env_step at n envs: action i32 [n] | reward f32 [n] | out-of-range word u32 [4] | done u8 [n].  was: 4n + 4n + 16 + n
  {
    const Sec n1[] = {{4, 1}, {4, 1}, {4, 4}, {1, 1}};              // 0..4 | 16..20 | 32..48 | 48..49
    replay(n1, 4, 49, 25);
    const Sec n3[] = {{4, 3}, {4, 3}, {4, 4}, {1, 3}};              // 0..12 | 16..28 | 32..48 | 48..51
    replay(n3, 4, 51, 43);
  }
  // crl_dqn_dueling_streams with R rows per stream: obs f64 [4n] | value f64 [Rn] | advantage f64 [2Rn].  was: 8n(4 + 3R)
  {
    const Sec r1n1[] = {{8, 4}, {8, 1}, {8, 2}};                    // scalar head: 0..32 | 32..40 | 48..64
    replay(r1n1, 3, 64, 56);
    const Sec r1n3[] = {{8, 12}, {8, 3}, {8, 6}};                   // 0..96 | 96..120 | 128..176
    replay(r1n3, 3, 176, 168);
    const Sec r51n1[] = {{8, 4}, {8, 51}, {8, 102}};                // 51 rows: 0..32 | 32..440 | 448..1264
    replay(r51n1, 3, 1264, 1256);
    const Sec r51n3[] = {{8, 12}, {8, 153}, {8, 306}};              // 0..96 | 96..1320 | 1328..3776
    replay(r51n3, 3, 3776, 3768);
    const Sec r2n1[] = {{8, 4}, {8, 2}, {8, 4}};                    // every section a multiple of 16 bytes: the totals agree
    replay(r2n1, 3, 80, 80);
    const Sec r2n3[] = {{8, 12}, {8, 6}, {8, 12}};
    replay(r2n3, 3, 240, 240);
  }
  std::puts("stage layout OK");
  return 0;
}
"""


def test_stage_layout_under_the_sanitizers(tmp_path):
    src = tmp_path / "stage_layout_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "stage_layout_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "stage layout OK"


def test_layout_header_is_free_of_hip():
    """the header the program above includes must stay plain C++: it names no HIP header and no other project header"""
    text = open(os.path.join(CSRC, "stage_layout.hpp")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"], includes
