// The wave-exchange reduction of fused_chunk (edge_alignment_amd/csrc/ea_wave_exchange.h) replayed on the host: a stand-alone
// program (built by tests/test_wave_exchange_host.py with -fsanitize=address,undefined) that runs both exchange rounds and the
// 8-value butterfly on SYMBOLIC values -- a value is the set of (wave, lane) whose entry of a slot went into it, tagged with
// the slot -- for all 4 waves x 64 lanes, with the header's ownership and layout arithmetic, and checks what the kernel relies
// on.  Every LDS cell keeps a log of its accesses (round, kind, wave), from which the ordering properties are checked under
// the only ordering the kernel has: program order inside a wave, and the barrier that closes a round's stores.
// Exit status 0 and "ok <slots>" on success; the first violated property is printed and the status is 1.
#include <bitset>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ea_wave_exchange.h"

using namespace ea;

struct Sym {
  int slot = -1;            // -1: never written
  std::bitset<256> from;    // (wave * 64 + lane) of the entries summed into it
};
static bool failed = false;
static void fail(const char *what, int a, int b, int c) {
  if (!failed) std::printf("FAILED: %s (%d, %d, %d)\n", what, a, b, c);
  failed = true;
}
static Sym add(const Sym &a, const Sym &b) {
  Sym r;
  if (a.slot < 0 || b.slot < 0) { fail("sum of a value that was never written", a.slot, b.slot, 0); return r; }
  if (a.slot != b.slot) fail("sum across two slots", a.slot, b.slot, 0);
  if ((a.from & b.from).any()) fail("an entry summed twice", a.slot, 0, 0);
  r.slot = a.slot; r.from = a.from | b.from;
  return r;
}

// the LDS array in 8-byte cells, each with its access log; phases: 0 = round-1 stores, 1 = round-1 loads (behind barrier 1),
// 2 = round-2 stores (no barrier in front!), 3 = round-2 loads (behind barrier 2)
struct Access { int phase, wave; };
struct Cell { Sym v; std::vector<Access> log; };
static std::vector<Cell> lds(kXchgBytes / 8);

static Cell &cell(int region, int j, int lane) {
  const int off = xchg_cell_offset(region, j, lane);
  if (off < 0 || off + 8 > kXchgBytes || off % 8) { fail("cell outside the exchange buffer", region, j, lane); std::exit(1); }
  return lds[(size_t)off / 8];
}

int main() {
  static Sym v[4][64][32], k[4][64][16], e[4][64][8];
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l)
      for (int s = 0; s < 32; ++s) { v[w][l][s].slot = s; v[w][l][s].from.set((size_t)w * 64 + l); }
  // 16-byte accesses: cells 2p, 2p + 1 of a lane are adjacent and aligned, the 64 lanes of an access contiguous
  for (int r = 0; r < 4; ++r)
    for (int p = 0; p < 8; ++p)
      for (int l = 0; l < 64; ++l) {
        const int o = xchg_cell_offset(r, 2 * p, l);
        if (o % 16 || xchg_cell_offset(r, 2 * p + 1, l) != o + 8) fail("cell pair is not one aligned 16-byte access", r, p, l);
        if (l && o != xchg_cell_offset(r, 2 * p, l - 1) + 16) fail("lanes of an access are not contiguous", r, p, l);
      }
  // ---- round 1: stores, barrier, loads
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 16; ++j) {
        Cell &c = cell(xchg_write_region1(w), j, l);
        c.v = v[w][l][xchg_send16(w) + j];
        c.log.push_back({0, w});
        k[w][l][j] = v[w][l][xchg_keep16(w) + j];
      }
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 16; ++j) {
        Cell &c = cell(xchg_read_region1(w), j, l);
        c.log.push_back({1, w});
        k[w][l][j] = add(k[w][l][j], c.v);
      }
  // ---- round 2: stores (8 cells), barrier, loads.  The stores come with no barrier behind the round-1 loads: a cell
  // stored now must have had this wave as its ONLY round-1 reader.
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        Cell &c = cell(xchg_write_region2(w), j, l);
        for (const Access &a : c.log)
          if (a.phase == 1 && a.wave != w) fail("round 2 writes a cell another wave still has to read", w, l, j);
        c.v = k[w][l][xchg_send8(w) + j];
        c.log.push_back({2, w});
        e[w][l][j] = k[w][l][xchg_keep8(w) + j];
      }
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        Cell &c = cell(xchg_read_region2(w), j, l);
        c.log.push_back({3, w});
        e[w][l][j] = add(e[w][l][j], c.v);
      }
  // ---- the logs: every load sees the last store of its own round -- in the log a load (phase 1 / 3) is preceded by exactly
  // one store of its round (phase 0 / 2), there is no store of that round behind it, and one writer per cell and round
  for (size_t i = 0; i < lds.size(); ++i) {
    const std::vector<Access> &log = lds[i].log;
    int stores[2] = {0, 0};
    for (size_t a = 0; a < log.size(); ++a) {
      const int round = log[a].phase >> 1;
      if (!(log[a].phase & 1)) {
        ++stores[round];
        for (size_t b = 0; b < a; ++b)
          if (log[b].phase == log[a].phase + 1) fail("a cell is read before its last write of the same round", (int)i, log[a].wave, round);
      } else if (stores[round] != 1) fail("a load without exactly one store of its round in front of it", (int)i, log[a].wave, round);
    }
    if (stores[0] > 1 || stores[1] > 1) fail("two stores to a cell in one round", (int)i, 0, 0);
  }
  // behind round 2 wave w holds slots [xchg_first_slot(w), +8) in every lane, summed over the four waves
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        const Sym &s = e[w][l][j];
        if (s.slot != xchg_first_slot(w) + j) fail("wave does not own the slot the header says", w, l, j);
        std::bitset<256> want;
        for (int u = 0; u < 4; ++u) want.set((size_t)u * 64 + l);
        if (s.from != want) fail("a lane's sum is not complete over the four waves", w, l, j);
      }
  // ---- the butterfly over 8 values, per wave
  int stored[32] = {0};
  int slots_done = 0;
  for (int w = 0; w < 4; ++w) {
    Sym a[64][4], b[64][2], c[64], d[64];
    // L ^ 32: the swap hands the upper half-wave's entry of value i to lane L - 32 and the lower half-wave's entry of value
    // i + 4 to lane L + 32; the lower half keeps i, the upper i + 4
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 4; ++i) a[l][i] = l < 32 ? add(e[w][l][i], e[w][l + 32][i]) : add(e[w][l - 32][i + 4], e[w][l][i + 4]);
    // L ^ 16: even rows keep i, odd rows i + 2
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 2; ++i) b[l][i] = !(l & 16) ? add(a[l][i], a[l + 16][i]) : add(a[l - 16][i + 2], a[l][i + 2]);
    // L ^ 15 with the select: bit 3 picks the value kept, the other one goes to the mirror lane of the row
    for (int l = 0; l < 64; ++l) {
      const int m = (l & ~15) | (15 - (l & 15));
      const bool upper = (l & 8) != 0, m_upper = (m & 8) != 0;
      c[l] = add(upper ? b[l][1] : b[l][0], m_upper ? b[m][0] : b[m][1]);
    }
    // three levels that add the partner's value: L ^ 7, L ^ 2, L ^ 1
    for (int x : {7, 2, 1}) {
      for (int l = 0; l < 64; ++l) d[l] = add(c[l], c[l ^ x]);
      for (int l = 0; l < 64; ++l) c[l] = d[l];
    }
    for (int l = 0; l < 64; ++l) {
      if (c[l].slot != xchg_first_slot(w) + xchg_lane_value(l)) fail("lane holds another slot than the header says", w, l, c[l].slot);
      const int s = xchg_store_slot(w, l);
      if (s < 0) continue;
      if (s >= 32 || s != c[l].slot) { fail("storing lane and slot disagree", w, l, s); continue; }
      if (c[l].from.count() != 256) fail("a stored sum is not the union of all 256 lanes' entries", w, l, s);
      ++stored[s];
    }
  }
  for (int s = 0; s < 32; ++s) {
    if (stored[s] != 1) fail("a slot does not end in exactly one storing lane", s, stored[s], 0);
    else ++slots_done;
  }
  if (failed) return 1;
  std::printf("ok %d\n", slots_done);
  return 0;
}
