// ppmd7_device.h -- PPMd7 (PPMd var.H) decoder for one stream: the model, its
// sub-allocator and the 7z range decoder, as one struct whose scalar state is
// meant to live in registers.  A restatement of what Ppmd7.c / Ppmd7Dec.c and
// SzDecodePpmd (7zDec.c:66-122) compute; every decision of the allocator is the
// reference's, because the model restarts when memory runs out and the decoded
// bytes therefore depend on which allocation fails.  The encoder (Ppmd7Enc.c:
// struct Ppmd7Enc at the end) derives from it and shares everything after the
// choice of a state, update_found().
//
// Memory: the model is a byte array of `align_off + mem_size + 12` bytes
// (ppmd7_model_bytes) addressed by 32-bit offsets, 0 meaning "none" -- the
// reference's 64-bit layout: the text area grows up from align_off, units of 12
// bytes are handed out between units_start and align_off + mem_size, and the
// 12 bytes after that hold the list head GlueFreeBlocks needs.  Every unit
// offset is a multiple of 4 (align_off + mem_size is, and units are carved in
// steps of 12 from there), so context and free-node fields take 16/32-bit
// accesses; symbol states are 6 bytes at 2-byte alignment and take 8/16-bit
// accesses only.
//
// Hot per-stream tables (Ppmd7Hot) sit beside the model: LDS on the device.
// BinSumm is reached through its own pointer (the kernel keeps it in the
// stream's workspace slice, after the model).
//
// Lanes: on the device all lanes of the wave run this code on the same state
// (wave-uniform control flow, identical stores to identical addresses).  The
// bulk initialisations are dealt over the lanes (lane, nlanes) and followed by
// PPMD7_SYNC(), and so are the encoder's searches for its symbol
// (Ppmd7Enc::scan_states); the host build is lane 0 of 1.
//
// The input never steers an address: the range decoder only picks which of the
// model's own, consistent transitions is taken, so every offset stays inside
// the model for any input.  Scans over a context's states are additionally
// capped by its state count, and BinSumm / SEE indices are masked or built from
// bounded terms.
#pragma once

#include <stdint.h>

#ifdef PPMD7_HOST_EMU
#define PPMD7_FN inline
#define PPMD7_TOP inline
#define PPMD7_SYNC() ((void)0)
#else
#define PPMD7_FN __device__ inline
#define PPMD7_TOP __device__ __forceinline__  // into the kernel: its LDS pointers keep their address space
#define PPMD7_SYNC() __syncthreads()
#endif

constexpr uint32_t kPpmd7Unit = 12;       // bytes per allocation unit
constexpr uint32_t kPpmd7Lists = 38;      // size classes: 1..4, 6..12 by 2, 15..24 by 3, 28..128 by 4 units
constexpr uint32_t kPpmd7MaxFreq = 124;
constexpr uint32_t kPpmd7MinOrder = 2, kPpmd7MaxOrder = 64;
constexpr uint32_t kPpmd7MinMem = 1u << 11, kPpmd7MaxMem = 0xFFFFFFFFu - 36u;
constexpr uint32_t kPpmd7BinCells = 128 * 64;
constexpr uint32_t kPpmd7SeeCells = 25 * 16;  // cell kPpmd7SeeCells is the order-0 dummy
constexpr uint32_t kPpmd7RcTop = 1u << 24;

PPMD7_FN uint32_t ppmd7_align_off(uint32_t mem_size) { return 4u - (mem_size & 3u); }
PPMD7_FN uint64_t ppmd7_model_bytes(uint32_t mem_size) {
  return uint64_t(ppmd7_align_off(mem_size)) + mem_size + kPpmd7Unit;
}

struct Ppmd7See {
  uint16_t summ;
  uint8_t shift, count;
};

// per-stream hot tables (about 3.7 KiB)
struct Ppmd7Hot {
  uint32_t cand[256];  // unmasked states of the current escape level; reused
                       // as the state stack of the successor builder
  uint32_t free_list[kPpmd7Lists];
  Ppmd7See see[kPpmd7SeeCells + 1];
  uint8_t mask[256];   // 0xFF: symbol still possible, 0: excluded
  uint8_t units_of[kPpmd7Lists];  // size class -> units
  uint8_t class_of[128];          // units - 1 -> size class
  uint8_t see_row[256];           // unmasked states - 1 -> SEE row
  uint8_t esc_start[16];          // binary probability >> 10 -> escape count of a new context
  uint16_t bin_start[8];          // initial escape weight of a binary cell, by cell & 7
};

struct Ppmd7Out {
  int32_t res;
  uint64_t dest_len, src_len;
};

struct Ppmd7 {
  uint8_t* m;      // model memory
  Ppmd7Hot* h;
  uint16_t* bin;   // kPpmd7BinCells
  uint32_t lane, nlanes;

  uint32_t min_ctx, max_ctx, found;
  uint32_t order_fall, init_esc, prev_success, max_order, hi_flag;
  int32_t run_len, init_rl;
  uint32_t size, glue_count, lo_unit, hi_unit, text, units_start, align_off;

  uint32_t range, code;
  const uint8_t* src;
  uint64_t pos, len;
  bool extra;

  // ---------------------------------------------------------------- memory
  PPMD7_FN uint32_t r8(uint32_t o) const { return m[o]; }
  PPMD7_FN uint32_t r16(uint32_t o) const { return *(const uint16_t*)(m + o); }
  PPMD7_FN uint32_t r32(uint32_t o) const { return *(const uint32_t*)(m + o); }
  PPMD7_FN void w8(uint32_t o, uint32_t v) { m[o] = uint8_t(v); }
  PPMD7_FN void w16(uint32_t o, uint32_t v) { *(uint16_t*)(m + o) = uint16_t(v); }
  PPMD7_FN void w32(uint32_t o, uint32_t v) { *(uint32_t*)(m + o) = v; }

  // context: +0 state count, +2 frequency sum, +4 states, +8 suffix; a context
  // with one state keeps it in bytes 2..7
  PPMD7_FN uint32_t c_n(uint32_t c) const { return r16(c); }
  PPMD7_FN uint32_t c_sum(uint32_t c) const { return r16(c + 2); }
  PPMD7_FN uint32_t c_states(uint32_t c) const { return r32(c + 4); }
  PPMD7_FN uint32_t c_suffix(uint32_t c) const { return r32(c + 8); }
  // state: +0 symbol, +1 frequency, +2 successor (two halves)
  PPMD7_FN uint32_t s_sym(uint32_t s) const { return r8(s); }
  PPMD7_FN uint32_t s_freq(uint32_t s) const { return r8(s + 1); }
  PPMD7_FN uint32_t s_succ(uint32_t s) const { return r16(s + 2) | (r16(s + 4) << 16); }
  PPMD7_FN void s_set_succ(uint32_t s, uint32_t v) {
    w16(s + 2, v & 0xFFFFu);
    w16(s + 4, v >> 16);
  }
  PPMD7_FN void s_copy(uint32_t to, uint32_t from) {
    const uint32_t a = r16(from), b = r16(from + 2), c = r16(from + 4);
    w16(to, a);
    w16(to + 2, b);
    w16(to + 4, c);
  }
  PPMD7_FN void s_swap(uint32_t x, uint32_t y) {
    const uint32_t a = r16(x), b = r16(x + 2), c = r16(x + 4);
    s_copy(x, y);
    w16(y, a);
    w16(y + 2, b);
    w16(y + 4, c);
  }
  PPMD7_FN void units_copy(uint32_t to, uint32_t from, uint32_t units) {
    for (uint32_t k = 0; k < units * 3; ++k) w32(to + 4 * k, r32(from + 4 * k));
  }
  PPMD7_FN static uint32_t high_flag(uint32_t sym) { return sym >= 0x40 ? 8u : 0u; }

  // ---------------------------------------------------------------- sub-allocator
  PPMD7_FN void list_push(uint32_t at, uint32_t cls) {
    w32(at, h->free_list[cls]);
    h->free_list[cls] = at;
  }
  PPMD7_FN uint32_t list_pop(uint32_t cls) {
    const uint32_t at = h->free_list[cls];
    h->free_list[cls] = r32(at);
    return at;
  }
  // free `units` units at `at`: as one block if a class has that size, else as
  // the next smaller class plus the remainder (1..3 units)
  PPMD7_FN void give_back(uint32_t at, uint32_t units) {
    uint32_t cls = h->class_of[units - 1];
    if (h->units_of[cls] != units) {
      const uint32_t k = h->units_of[--cls];
      list_push(at + k * kPpmd7Unit, units - k - 1);
    }
    list_push(at, cls);
  }
  // keep the first units_of[keep] units of a block of class `whole`
  PPMD7_FN void split_tail(uint32_t at, uint32_t whole, uint32_t keep) {
    give_back(at + h->units_of[keep] * kPpmd7Unit, h->units_of[whole] - h->units_of[keep]);
  }

  // Merge adjacent free blocks: thread all of them on a doubly linked list
  // (node: +0 stamp, 0 = free; +2 units; +4 next; +8 prev) whose head is the
  // 12 bytes after the units area, merge each with the free blocks that follow
  // it while the sum stays below 65536 units, and deal the results out again.
  PPMD7_FN void glue_free_blocks() {
    const uint32_t head = align_off + size;
    uint32_t n = head;
    glue_count = 255;
    for (uint32_t cls = 0; cls < kPpmd7Lists; ++cls) {
      const uint32_t units = h->units_of[cls];
      uint32_t next = h->free_list[cls];
      h->free_list[cls] = 0;
      while (next != 0) {
        const uint32_t node = next;
        w32(node + 4, n);
        w32(n + 8, node);
        n = node;
        next = r32(node);
        w16(node, 0);
        w16(node + 2, units);
      }
    }
    w16(head, 1);
    w32(head + 4, n);
    w32(n + 8, head);
    if (lo_unit != hi_unit) w16(lo_unit, 1);

    while (n != head) {
      uint32_t units = r16(n + 2);
      for (;;) {
        const uint32_t after = n + units * kPpmd7Unit;
        units += r16(after + 2);
        if (r16(after) != 0 || units >= 0x10000u) break;
        const uint32_t an = r32(after + 4), ap = r32(after + 8);
        w32(ap + 4, an);
        w32(an + 8, ap);
        w16(n + 2, units);
      }
      n = r32(n + 4);
    }

    for (n = r32(head + 4); n != head;) {
      const uint32_t next = r32(n + 4);
      uint32_t units = r16(n + 2), at = n;
      for (; units > 128; units -= 128, at += 128 * kPpmd7Unit) list_push(at, kPpmd7Lists - 1);
      give_back(at, units);
      n = next;
    }
  }

  // the slow path: glue, then a larger block cut down, then the gap between the
  // text and the units area; 0 when all fail
  PPMD7_FN uint32_t alloc_rare(uint32_t cls) {
    if (glue_count == 0) {
      glue_free_blocks();
      if (h->free_list[cls] != 0) return list_pop(cls);
    }
    uint32_t big = cls;
    do {
      if (++big == kPpmd7Lists) {
        const uint32_t bytes = h->units_of[cls] * kPpmd7Unit;
        --glue_count;
        if (units_start - text > bytes) return units_start -= bytes;
        return 0;
      }
    } while (h->free_list[big] == 0);
    const uint32_t at = list_pop(big);
    split_tail(at, big, cls);
    return at;
  }
  PPMD7_FN uint32_t alloc_units(uint32_t cls) {
    if (h->free_list[cls] != 0) return list_pop(cls);
    const uint32_t bytes = h->units_of[cls] * kPpmd7Unit;
    if (bytes <= hi_unit - lo_unit) {
      const uint32_t at = lo_unit;
      lo_unit += bytes;
      return at;
    }
    return alloc_rare(cls);
  }
  PPMD7_FN uint32_t alloc_context() {
    if (hi_unit != lo_unit) return hi_unit -= kPpmd7Unit;
    if (h->free_list[0] != 0) return list_pop(0);
    return alloc_rare(0);
  }
  PPMD7_FN uint32_t shrink_units(uint32_t at, uint32_t old_units, uint32_t new_units) {
    const uint32_t c0 = h->class_of[old_units - 1], c1 = h->class_of[new_units - 1];
    if (c0 == c1) return at;
    if (h->free_list[c1] != 0) {
      const uint32_t to = list_pop(c1);
      units_copy(to, at, new_units);
      list_push(at, c0);
      return to;
    }
    split_tail(at, c0, c1);
    return at;
  }

  // ---------------------------------------------------------------- model
  // constant tables; once per Ppmd7Hot
  PPMD7_FN void build_tables() {
    uint32_t k = 0;
    for (uint32_t cls = 0; cls < kPpmd7Lists; ++cls) {
      const uint32_t step = cls >= 12 ? 4 : (cls >> 2) + 1;
      for (uint32_t j = 0; j < step; ++j) h->class_of[k++] = uint8_t(cls);
      h->units_of[cls] = uint8_t(k);
    }
    // SEE row by unmasked count: 0, 1, 2, then row r repeated r - 1 times
    uint32_t row = 3, left = 1;
    for (uint32_t i = 0; i < 256; ++i) {
      if (i < 3) {
        h->see_row[i] = uint8_t(i);
        continue;
      }
      h->see_row[i] = uint8_t(row);
      if (--left == 0) left = ++row - 2;
    }
    const uint8_t esc[16] = {25, 14, 9, 7, 5, 5, 4, 4, 4, 3, 3, 3, 2, 2, 2, 2};
    const uint16_t b0[8] = {0x3CDD, 0x1F3F, 0x59BF, 0x48F3, 0x64A1, 0x5ABC, 0x6632, 0x6051};
    for (uint32_t i = 0; i < 16; ++i) h->esc_start[i] = esc[i];
    for (uint32_t i = 0; i < 8; ++i) h->bin_start[i] = b0[i];
    PPMD7_SYNC();
  }

  PPMD7_FN void restart_model() {
    for (uint32_t i = 0; i < kPpmd7Lists; ++i) h->free_list[i] = 0;
    text = align_off;
    hi_unit = text + size;
    lo_unit = units_start = hi_unit - size / 8 / kPpmd7Unit * 7 * kPpmd7Unit;
    glue_count = 0;
    order_fall = max_order;
    run_len = init_rl = -int32_t(max_order < 12 ? max_order : 12) - 1;
    prev_success = 0;

    hi_unit -= kPpmd7Unit;
    min_ctx = max_ctx = hi_unit;
    found = lo_unit;
    lo_unit += 128 * kPpmd7Unit;
    w16(min_ctx, 256);
    w16(min_ctx + 2, 257);
    w32(min_ctx + 4, found);
    w32(min_ctx + 8, 0);
    for (uint32_t i = lane; i < 256; i += nlanes) {
      const uint32_t s = found + 6 * i;
      w16(s, i | (1u << 8));  // symbol i, frequency 1
      w16(s + 2, 0);
      w16(s + 4, 0);
    }
    for (uint32_t j = lane; j < kPpmd7BinCells; j += nlanes)
      bin[j] = uint16_t(16384u - uint32_t(h->bin_start[j & 7]) / ((j >> 6) + 2));
    for (uint32_t j = lane; j < kPpmd7SeeCells; j += nlanes) {
      Ppmd7See v;
      v.shift = 3;
      v.summ = uint16_t((5 * (j >> 4) + 10) << 3);
      v.count = 4;
      h->see[j] = v;
    }
    PPMD7_SYNC();
  }

  PPMD7_FN void init_model(uint32_t order, uint32_t mem_size) {
    size = mem_size;
    align_off = ppmd7_align_off(mem_size);
    max_order = order;
    init_esc = 0;
    hi_flag = 0;
    restart_model();
    Ppmd7See d;
    d.shift = 7;
    d.summ = 0;
    d.count = 64;
    h->see[kPpmd7SeeCells] = d;
    PPMD7_SYNC();
  }

  // state of `sym` in context c, which holds it (capped by the state count)
  PPMD7_FN uint32_t find_state(uint32_t c, uint32_t sym) const {
    uint32_t s = c_states(c);
    for (uint32_t left = c_n(c); left > 1 && s_sym(s) != sym; --left) s += 6;
    return s;
  }

  // Contexts for the found symbol along the suffix chain that do not have one
  // yet; returns the longest, or 0 when memory ran out.
  PPMD7_FN uint32_t create_successors(bool skip) {
    uint32_t c = min_ctx;
    const uint32_t up = s_succ(found), fsym = s_sym(found);
    uint32_t* stack = h->cand;
    uint32_t depth = 0;
    if (!skip) stack[depth++] = found;
    while (c_suffix(c) != 0) {
      c = c_suffix(c);
      const uint32_t s = c_n(c) != 1 ? find_state(c, fsym) : c + 2;
      const uint32_t next = s_succ(s);
      if (next != up) {
        c = next;
        if (depth == 0) return c;
        break;
      }
      stack[depth++ & 255u] = s;
    }
    const uint32_t up_sym = r8(up);
    uint32_t up_freq;
    if (c_n(c) == 1) {
      up_freq = s_freq(c + 2);
    } else {
      const uint32_t cf = s_freq(find_state(c, up_sym)) - 1;
      const uint32_t s0 = c_sum(c) - c_n(c) - cf;
      up_freq = 1 + (2 * cf <= s0 ? uint32_t(5 * cf > s0) : (2 * cf + 3 * s0 - 1) / (2 * s0));
    }
    while (depth != 0) {
      const uint32_t c1 = alloc_context();
      if (c1 == 0) return 0;
      w16(c1, 1);
      w16(c1 + 2, up_sym | ((up_freq & 0xFFu) << 8));
      s_set_succ(c1 + 2, up + 1);
      w32(c1 + 8, c);
      s_set_succ(stack[--depth & 255u], c1);
      c = c1;
    }
    return c;
  }

  // false: memory ran out, the caller restarts the model
  PPMD7_FN bool update_model() {
    const uint32_t fsym = s_sym(found), ffreq = s_freq(found);
    uint32_t fsucc = s_succ(found);
    if (ffreq < kPpmd7MaxFreq / 4 && c_suffix(min_ctx) != 0) {
      const uint32_t c = c_suffix(min_ctx);
      if (c_n(c) == 1) {
        const uint32_t f = s_freq(c + 2);
        if (f < 32) w8(c + 3, f + 1);
      } else {
        uint32_t s = c_states(c);
        if (s_sym(s) != fsym) {
          s = find_state(c, fsym);
          if (s_freq(s) >= s_freq(s - 6)) {
            s_swap(s, s - 6);
            s -= 6;
          }
        }
        const uint32_t f = s_freq(s);
        if (f < kPpmd7MaxFreq - 9) {
          w8(s + 1, f + 2);
          w16(c + 2, c_sum(c) + 2);
        }
      }
    }

    if (order_fall == 0) {
      const uint32_t c = create_successors(true);
      min_ctx = max_ctx = c;
      if (c == 0) return false;
      s_set_succ(found, c);
      return true;
    }

    w8(text++, fsym);
    uint32_t successor = text;
    if (text >= units_start) return false;

    if (fsucc != 0) {
      if (fsucc <= successor) {
        const uint32_t c = create_successors(false);
        if (c == 0) return false;
        fsucc = c;
      }
      if (--order_fall == 0) {
        successor = fsucc;
        text -= (max_ctx != min_ctx) ? 1u : 0u;
      }
    } else {
      s_set_succ(found, successor);
      fsucc = min_ctx;
    }

    const uint32_t ns = c_n(min_ctx);
    const uint32_t s0 = c_sum(min_ctx) - ns - (ffreq - 1);
    for (uint32_t c = max_ctx; c != min_ctx; c = c_suffix(c)) {
      const uint32_t ns1 = c_n(c);
      uint32_t sum;
      if (ns1 != 1) {
        if ((ns1 & 1) == 0) {
          // the states fill their units: move to the next class if one more
          // unit is one
          const uint32_t units = ns1 >> 1;
          const uint32_t cls = h->class_of[units - 1];
          if (cls != h->class_of[units & 127u]) {
            const uint32_t to = alloc_units(cls + 1);
            if (to == 0) return false;
            const uint32_t from = c_states(c);
            units_copy(to, from, units);
            list_push(from, cls);
            w32(c + 4, to);
          }
        }
        sum = c_sum(c);
        sum = (sum + (2 * ns1 < ns) + 2 * ((4 * ns1 <= ns) & (sum <= 8 * ns1))) & 0xFFFFu;
      } else {
        const uint32_t s = alloc_units(0);
        if (s == 0) return false;
        s_copy(s, c + 2);
        w32(c + 4, s);
        uint32_t f = s_freq(s);
        f = f < kPpmd7MaxFreq / 4 - 1 ? f << 1 : kPpmd7MaxFreq - 4;
        w8(s + 1, f);
        sum = (f + init_esc + (ns > 3)) & 0xFFFFu;
      }
      uint32_t cf = 2 * ffreq * (sum + 6);
      const uint32_t sf = s0 + sum;
      if (cf < 6 * sf) {
        cf = 1 + (cf > sf) + (cf >= 4 * sf);
        sum += 3;
      } else {
        cf = 4 + (cf >= 9 * sf) + (cf >= 12 * sf) + (cf >= 15 * sf);
        sum += cf;
      }
      w16(c + 2, sum);
      const uint32_t s = c_states(c) + 6 * ns1;
      w16(s, fsym | (cf << 8));
      s_set_succ(s, successor);
      w16(c, ns1 + 1);
    }
    max_ctx = min_ctx = fsucc;
    return true;
  }

  // halve the frequencies of the current context, keeping its states sorted;
  // states that reach 0 are dropped
  PPMD7_FN void rescale() {
    const uint32_t ns = c_n(min_ctx);
    if (ns < 2) return;
    const uint32_t stats = c_states(min_ctx);
    uint32_t s = found;
    {
      const uint32_t a = r16(s), b = r16(s + 2), c = r16(s + 4);
      for (; s != stats; s -= 6) s_copy(s, s - 6);
      w16(s, a);
      w16(s + 2, b);
      w16(s + 4, c);
    }
    uint32_t esc = c_sum(min_ctx) - s_freq(s);
    const uint32_t adder = order_fall != 0 ? 1u : 0u;
    uint32_t f = (((s_freq(s) + 4) & 0xFFu) + adder) >> 1;
    w8(s + 1, f);
    uint32_t sum = f;
    uint32_t i = ns - 1;
    do {
      s += 6;
      esc -= s_freq(s);
      f = (s_freq(s) + adder) >> 1;
      w8(s + 1, f);
      sum += f;
      if (f > s_freq(s - 6)) {
        const uint32_t a = r16(s), b = r16(s + 2), c = r16(s + 4);
        uint32_t t = s;
        do {
          s_copy(t, t - 6);
          t -= 6;
        } while (t != stats && f > s_freq(t - 6));
        w16(t, a);
        w16(t + 2, b);
        w16(t + 4, c);
      }
    } while (--i);

    if (s_freq(s) == 0) {
      uint32_t gone = 0;
      do {
        ++gone;
        s -= 6;
      } while (s_freq(s) == 0);
      esc += gone;
      const uint32_t left = ns - gone;
      w16(min_ctx, left);
      if (left == 1) {
        const uint32_t sym = s_sym(stats), succ = s_succ(stats);
        uint32_t tf = s_freq(stats);
        do {
          tf -= tf >> 1;
          esc >>= 1;
        } while (esc > 1);
        list_push(stats, h->class_of[((ns + 1) >> 1) - 1]);
        found = min_ctx + 2;
        w16(found, sym | (tf << 8));
        s_set_succ(found, succ);
        return;
      }
      const uint32_t n0 = (ns + 1) >> 1, n1 = (left + 1) >> 1;
      if (n0 != n1) w32(min_ctx + 4, shrink_units(stats, n0, n1));
    }
    w16(min_ctx + 2, sum + esc - (esc >> 1));
    found = c_states(min_ctx);
  }

  // SEE cell for an escape from the current context with `masked` symbols
  // excluded, and its escape estimate
  PPMD7_FN uint32_t escape_estimate(uint32_t masked, uint32_t& esc) {
    const uint32_t ns = c_n(min_ctx);
    if (ns == 256) {
      esc = 1;
      return kPpmd7SeeCells;
    }
    const uint32_t open = ns - masked;
    const uint32_t cell = uint32_t(h->see_row[(open - 1) & 255u]) * 16 +
                          (open < c_n(c_suffix(min_ctx)) - ns) + 2 * (c_sum(min_ctx) < 11 * ns) +
                          4 * (masked > open) + hi_flag;
    Ppmd7See v = h->see[cell];
    const uint32_t r = v.summ >> v.shift;
    v.summ = uint16_t(v.summ - r);
    h->see[cell] = v;
    esc = r + (r == 0);
    return cell;
  }

  // BinSumm cell of the one-state context whose state is s (Ppmd7_GetBinSumm);
  // sets hi_flag as the reference's macro does
  PPMD7_FN uint32_t bin_cell(uint32_t s) {
    const uint32_t f = s_freq(s);
    hi_flag = high_flag(s_sym(found));
    const uint32_t up = c_n(c_suffix(min_ctx)) - 1;
    const uint32_t by_up = up == 0 ? 0u : up == 1 ? 2u : up < 11 ? 4u : 6u;
    return (((f - 1) << 6) + prev_success + by_up + hi_flag + 2 * high_flag(s_sym(s)) +
            ((uint32_t(run_len >> 26)) & 0x20u)) &
           (kPpmd7BinCells - 1);
  }

  // how `found` was reached in min_ctx
  enum How : uint32_t { kFirst, kOther, kBinary, kEscaped };

  // Everything after the state is chosen, for both directions: Ppmd7_Update1_0
  // / Update1 / UpdateBin / Update2 with Rescale, then NextContext's successor
  // shortcut or UpdateModel, and the restart when memory ran out.
  PPMD7_FN void update_found(How how) {
    bool need_rescale = false;
    if (how == kBinary) {
      const uint32_t f = s_freq(found);
      w8(found + 1, f + (f < 128 ? 1 : 0));
      prev_success = 1;
      ++run_len;
    } else {
      uint32_t f = s_freq(found);
      const uint32_t sum = c_sum(min_ctx);
      if (how == kFirst) {
        prev_success = 2 * f > sum ? 1u : 0u;
        run_len += int32_t(prev_success);
      }
      f = (f + 4) & 0xFFu;
      w8(found + 1, f);
      w16(min_ctx + 2, sum + 4);
      if (how == kOther) {
        if (f > s_freq(found - 6)) {
          s_swap(found, found - 6);
          found -= 6;
          need_rescale = f > kPpmd7MaxFreq;
        }
      } else {
        need_rescale = f > kPpmd7MaxFreq;
      }
    }
    if (need_rescale) rescale();
    bool follow = false;
    uint32_t next = 0;
    if (how == kEscaped) {
      run_len = init_rl;
    } else if (order_fall == 0) {
      next = s_succ(found);
      follow = next > text;
    }
    if (follow)
      min_ctx = max_ctx = next;
    else if (!update_model())
      restart_model();
  }

  // ---------------------------------------------------------------- range decoder
  PPMD7_FN uint32_t read_byte() {
    if (pos < len) return src[pos++];
    extra = true;
    return 0;
  }
  PPMD7_FN void rc_normalize() {
    if (range < kPpmd7RcTop) {
      code = (code << 8) | read_byte();
      range <<= 8;
      if (range < kPpmd7RcTop) {
        code = (code << 8) | read_byte();
        range <<= 8;
      }
    }
  }
  PPMD7_FN uint32_t rc_threshold(uint32_t total) {
    range /= total;
    return code / range;
  }
  PPMD7_FN void rc_take(uint32_t start, uint32_t width) {
    code -= start * range;
    range *= width;
    rc_normalize();
  }
  // false: the stream cannot start (first byte, or the all-ones code)
  PPMD7_FN bool rc_init() {
    code = 0;
    range = 0xFFFFFFFFu;
    if (read_byte() != 0) return false;
    for (int i = 0; i < 4; ++i) code = (code << 8) | read_byte();
    return code < 0xFFFFFFFFu;
  }

  PPMD7_FN void mask_all() {
    uint32_t* w = (uint32_t*)h->mask;
    for (uint32_t j = lane; j < 64; j += nlanes) w[j] = 0xFFFFFFFFu;
    PPMD7_SYNC();
  }

  // one symbol: 0..255, -1 end of the suffix chain, -2 a count outside the
  // model's total
  PPMD7_FN int decode_symbol() {
    How how = kEscaped;
    const uint32_t ns0 = c_n(min_ctx);
    bool escaped = false;
    if (ns0 != 1) {
      uint32_t s = c_states(min_ctx);
      const uint32_t total = c_sum(min_ctx);
      const uint32_t count = rc_threshold(total);
      uint32_t hi = s_freq(s);
      if (count < hi) {
        rc_take(0, hi);
        found = s;
        how = kFirst;
      } else {
        prev_success = 0;
        uint32_t f = 0;
        bool hit = false;
        for (uint32_t i = ns0 - 1; i != 0; --i) {
          s += 6;
          f = s_freq(s);
          hi += f;
          if (hi > count) {
            hit = true;
            break;
          }
        }
        if (hit) {
          rc_take(hi - f, f);
          found = s;
          how = kOther;
        } else {
          if (count >= total) return -2;
          hi_flag = high_flag(s_sym(found));
          rc_take(hi, total - hi);
          mask_all();
          for (uint32_t i = ns0; i != 0; --i, s -= 6) h->mask[s_sym(s)] = 0;
          escaped = true;
          how = kEscaped;
        }
      }
    } else {
      const uint32_t s = min_ctx + 2;
      const uint32_t cell = bin_cell(s);
      const uint32_t pr = bin[cell];
      const uint32_t bound = (range >> 14) * pr;
      if (code < bound) {
        range = bound;
        rc_normalize();
        bin[cell] = uint16_t(pr + 128 - ((pr + 32) >> 7));
        found = s;
        how = kBinary;
      } else {
        code -= bound;
        range -= bound;
        rc_normalize();
        const uint32_t np = pr - ((pr + 32) >> 7);
        bin[cell] = uint16_t(np);
        init_esc = h->esc_start[(np >> 10) & 15u];
        mask_all();
        h->mask[s_sym(s)] = 0;
        prev_success = 0;
        escaped = true;
        how = kEscaped;
      }
    }

    while (escaped) {
      const uint32_t masked = c_n(min_ctx);
      do {
        ++order_fall;
        const uint32_t up = c_suffix(min_ctx);
        if (up == 0) return -1;
        min_ctx = up;
      } while (c_n(min_ctx) == masked);
      const uint32_t ns = c_n(min_ctx);
      const uint32_t open = ns - masked;
      uint32_t hi = 0, n = 0;
      uint32_t s = c_states(min_ctx);
      for (uint32_t left = ns; left != 0 && n != open; --left, s += 6) {
        if (h->mask[s_sym(s)] != 0) {
          hi += s_freq(s);
          h->cand[n++] = s;
        }
      }
      uint32_t esc;
      const uint32_t cell = escape_estimate(masked, esc);
      const uint32_t total = esc + hi;
      const uint32_t count = rc_threshold(total);
      if (count < hi) {
        uint32_t j = 0, acc = s_freq(h->cand[0]);
        while (acc <= count && j + 1 < n) acc += s_freq(h->cand[++j]);
        s = h->cand[j];
        const uint32_t f = s_freq(s);
        rc_take(acc - f, f);
        Ppmd7See v = h->see[cell];
        if (v.shift < 7 && --v.count == 0) {
          v.summ = uint16_t(v.summ << 1);
          v.count = uint8_t(3u << v.shift++);
        }
        h->see[cell] = v;
        found = s;
        break;
      }
      if (count >= total) return -2;
      rc_take(hi, total - hi);
      h->see[cell].summ = uint16_t(h->see[cell].summ + total);
      for (uint32_t j = 0; j < n; ++j) h->mask[s_sym(h->cand[j])] = 0;
    }

    const uint32_t symbol = s_sym(found);
    update_found(how);
    return int(symbol);
  }
};

// SzDecodePpmd over a memory buffer (7zDec.c:66-122): `hot` and `bin` are this
// stream's tables (hot built by Ppmd7::build_tables), `model` its
// ppmd7_model_bytes(mem_size) bytes, 4-byte aligned.
PPMD7_TOP Ppmd7Out ppmd7_decode_stream(const uint8_t* src, uint64_t src_len, uint8_t* dst,
                                      uint64_t dst_len, uint32_t order, uint32_t mem_size,
                                      uint8_t* model, Ppmd7Hot* hot, uint16_t* bin, uint32_t lane,
                                      uint32_t nlanes) {
  Ppmd7Out out;
  out.dest_len = 0;
  out.src_len = 0;
  if (order < kPpmd7MinOrder || order > kPpmd7MaxOrder || mem_size < kPpmd7MinMem ||
      mem_size > kPpmd7MaxMem) {
    out.res = 4;  // SZ_ERROR_UNSUPPORTED
    return out;
  }
  Ppmd7 p;
  p.m = model;
  p.h = hot;
  p.bin = bin;
  p.lane = lane;
  p.nlanes = nlanes;
  p.src = src;
  p.pos = 0;
  p.len = src_len;
  p.extra = false;
  out.res = 1;  // SZ_ERROR_DATA
  uint64_t i = 0;
  if (p.rc_init() && !p.extra) {
    if (dst_len != 0) p.init_model(order, mem_size);
    for (; i < dst_len; ++i) {
      const int sym = p.decode_symbol();
      if (p.extra || sym < 0) break;
      dst[i] = uint8_t(sym);
    }
    if (i == dst_len && p.pos == src_len && p.code == 0) out.res = 0;
  }
  out.dest_len = i;
  out.src_len = p.pos;
  return out;
}

// ---------------------------------------------------------------- encoder
// Ppmd7Enc.c on the same model: the 7z range encoder (Ppmd7Enc.c:9-72) and
// Ppmd7_EncodeSymbol (Ppmd7Enc.c:77-185).  The symbol only selects which state
// of the model's own contexts is taken, so, as in the decoder, no input byte
// steers an address.  The output position counts every byte of the stream;
// a byte is stored only while the position is below dst_cap.
#ifndef PPMD7_ENC_COUNT
#define PPMD7_ENC_COUNT(carry, pending) ((void)0)  // the host build counts carries here
#endif

struct Ppmd7EncOut {
  int32_t res;
  uint64_t dest_len, packed_len;
};

struct Ppmd7Enc : Ppmd7 {
  uint64_t low, cache_size;  // range is Ppmd7::range
  uint32_t cache;
  uint8_t* dst;
  uint64_t out_pos, dst_cap;

  PPMD7_FN void rc_enc_init() {
    low = 0;
    range = 0xFFFFFFFFu;
    cache = 0;
    cache_size = 1;
    out_pos = 0;
  }
  PPMD7_FN void put_byte(uint32_t b) {
    if (out_pos < dst_cap) dst[out_pos] = uint8_t(b);
    ++out_pos;
  }
  // RangeEnc_ShiftLow: the byte held back and the 0xFF bytes pending behind it
  // go out once a carry into them is decided
  PPMD7_FN void shift_low() {
    const uint32_t carry = uint32_t(low >> 32);
    if (uint32_t(low) < 0xFF000000u || carry != 0) {
      PPMD7_ENC_COUNT(carry, cache_size);
      uint32_t b = cache;
      do {
        put_byte((b + carry) & 0xFFu);
        b = 0xFF;
      } while (--cache_size != 0);
      cache = uint32_t(low) >> 24;
    }
    ++cache_size;
    low = uint64_t(uint32_t(low) << 8);
  }
  PPMD7_FN void rc_enc_normalize() {
    while (range < kPpmd7RcTop) {
      range <<= 8;
      shift_low();
    }
  }
  PPMD7_FN void rc_encode(uint32_t start, uint32_t width, uint32_t total) {
    range /= total;
    low += uint32_t(start * range);
    range *= width;
    rc_enc_normalize();
  }
  PPMD7_FN void rc_enc_flush() {
    for (int i = 0; i < 5; ++i) shift_low();
  }

  // The encoder knows its symbol, so a context's states are searched by all
  // lanes at once, lane l taking state l, l + nlanes, ...  Returns the
  // symbol's index among the ns states at `stats` (ns: absent) with `before`
  // the frequency sum in front of it (absent: of all).  kMasked: frequencies
  // count through the exclusion mask, every state's symbol is excluded as it
  // is passed and `whole` is the sum over all states; else the scan stops at
  // the hit.  Lane 0 of 1 runs this as the serial loop.
#ifdef PPMD7_HOST_EMU
  PPMD7_FN static uint64_t wave_ballot(bool p) { return p ? 1u : 0u; }
  PPMD7_FN static uint32_t wave_add(uint32_t v) { return v; }
#else
  PPMD7_FN static uint64_t wave_ballot(bool p) { return __ballot(p); }
  PPMD7_FN static uint32_t wave_add(uint32_t v) {
    for (int d = 32; d != 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
  }
#endif
  template <bool kMasked>
  PPMD7_FN uint32_t scan_states(uint32_t stats, uint32_t ns, uint32_t sym, uint32_t& before,
                                uint32_t& whole) {
    uint32_t hit = ns;
    before = whole = 0;
    for (uint32_t base = 0; base < ns; base += nlanes) {
      const uint32_t i = base + lane;
      const bool in = i < ns;
      const uint32_t w = in ? r16(stats + 6 * i) : 0u;  // symbol | frequency << 8
      const uint32_t cur = w & 0xFFu;
      uint32_t f = w >> 8;
      if (kMasked && in) {
        f &= h->mask[cur];
        h->mask[cur] = 0;
      }
      // one wave sum for both: a chunk's frequencies stay below 1 << 16
      uint32_t part = f << 16;
      if (hit == ns) {
        const uint64_t m = wave_ballot(in && cur == sym);
        if (m != 0) {
          const uint32_t pos = uint32_t(__builtin_ctzll(m));
          hit = base + pos;
          part |= lane < pos ? f : 0u;
        } else {
          part |= f;
        }
      }
      const uint32_t r = wave_add(part);
      before += r & 0xFFFFu;
      whole += r >> 16;
      if (!kMasked && hit != ns) break;
    }
    if (kMasked) PPMD7_SYNC();
    return hit;
  }

  // false: the suffix chain ended without the symbol (the reference's end-mark
  // return; the root context holds every byte, so no byte symbol gets here
  // with a consistent model)
  PPMD7_FN bool encode_symbol(uint32_t sym) {
    How how = kEscaped;
    const uint32_t ns0 = c_n(min_ctx);
    bool escaped = false;
    if (ns0 != 1) {
      const uint32_t stats = c_states(min_ctx), total = c_sum(min_ctx);
      uint32_t before, whole;
      const uint32_t at = scan_states<false>(stats, ns0, sym, before, whole);
      if (at == 0) {
        rc_encode(0, s_freq(stats), total);
        found = stats;
        how = kFirst;
      } else {
        prev_success = 0;
        if (at != ns0) {
          const uint32_t s = stats + 6 * at;
          rc_encode(before, s_freq(s), total);
          found = s;
          how = kOther;
        } else {
          hi_flag = high_flag(s_sym(found));
          mask_all();
          for (uint32_t i = lane; i < ns0; i += nlanes) h->mask[s_sym(stats + 6 * i)] = 0;
          PPMD7_SYNC();
          rc_encode(before, total - before, total);
          escaped = true;
        }
      }
    } else {
      const uint32_t s = min_ctx + 2;
      const uint32_t cell = bin_cell(s);
      const uint32_t pr = bin[cell];
      const uint32_t bound = (range >> 14) * pr;
      if (s_sym(s) == sym) {
        range = bound;
        rc_enc_normalize();
        bin[cell] = uint16_t(pr + 128 - ((pr + 32) >> 7));
        found = s;
        how = kBinary;
      } else {
        low += bound;
        range -= bound;
        rc_enc_normalize();
        const uint32_t np = pr - ((pr + 32) >> 7);
        bin[cell] = uint16_t(np);
        init_esc = h->esc_start[(np >> 10) & 15u];
        mask_all();
        h->mask[s_sym(s)] = 0;
        prev_success = 0;
        escaped = true;
      }
    }

    while (escaped) {
      const uint32_t masked = c_n(min_ctx);
      do {
        ++order_fall;
        const uint32_t up = c_suffix(min_ctx);
        if (up == 0) return false;
        min_ctx = up;
      } while (c_n(min_ctx) == masked);
      uint32_t esc;
      const uint32_t cell = escape_estimate(masked, esc);
      uint32_t before, sum;
      const uint32_t ns = c_n(min_ctx), stats = c_states(min_ctx);
      const uint32_t at = scan_states<true>(stats, ns, sym, before, sum);
      const uint32_t hit = at != ns ? stats + 6 * at : 0u;
      const uint32_t total = sum + esc;
      if (hit != 0) {
        rc_encode(before, s_freq(hit), total);
        Ppmd7See v = h->see[cell];
        if (v.shift < 7 && --v.count == 0) {
          v.summ = uint16_t(v.summ << 1);
          v.count = uint8_t(3u << v.shift++);
        }
        h->see[cell] = v;
        found = hit;
        break;
      }
      rc_encode(sum, esc, total);
      h->see[cell].summ = uint16_t(h->see[cell].summ + total);
    }
    update_found(how);
    return true;
  }
};

// Ppmd7z_RangeEnc_Init, Ppmd7_EncodeSymbol over src_len bytes and
// Ppmd7z_RangeEnc_FlushData, with no end mark (7z streams carry none).  `hot`,
// `bin` and `model` as for ppmd7_decode_stream.  res: 0; 5 (SZ_ERROR_PARAM) for
// order / mem_size out of range, nothing read or written; 7
// (SZ_ERROR_OUTPUT_EOF) when the stream is longer than dst_cap -- dst then
// holds its first dst_cap bytes and packed_len its whole length; 11
// (SZ_ERROR_FAIL) if a suffix chain ended without the symbol, the stream
// stopping there.
PPMD7_TOP Ppmd7EncOut ppmd7_encode_stream(const uint8_t* src, uint64_t src_len, uint8_t* dst,
                                         uint64_t dst_cap, uint32_t order, uint32_t mem_size,
                                         uint8_t* model, Ppmd7Hot* hot, uint16_t* bin,
                                         uint32_t lane, uint32_t nlanes) {
  Ppmd7EncOut out;
  out.dest_len = 0;
  out.packed_len = 0;
  if (order < kPpmd7MinOrder || order > kPpmd7MaxOrder || mem_size < kPpmd7MinMem ||
      mem_size > kPpmd7MaxMem) {
    out.res = 5;  // SZ_ERROR_PARAM
    return out;
  }
  Ppmd7Enc p;
  p.m = model;
  p.h = hot;
  p.bin = bin;
  p.lane = lane;
  p.nlanes = nlanes;
  p.dst = dst;
  p.dst_cap = dst_cap;
  p.rc_enc_init();
  if (src_len != 0) p.init_model(order, mem_size);
  bool ok = true;
  for (uint64_t i = 0; i < src_len && ok; ++i) ok = p.encode_symbol(src[i]);
  if (ok) p.rc_enc_flush();
  out.packed_len = p.out_pos;
  out.dest_len = p.out_pos < dst_cap ? p.out_pos : dst_cap;
  out.res = !ok ? 11 : p.out_pos > dst_cap ? 7 : 0;
  return out;
}
