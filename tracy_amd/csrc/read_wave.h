// read_wave.h -- readab (abif.h:286-405) and readscf (scf.h:38-102) of file images that lie in device memory, equal in every field to
// tracy_amd/host/trace_io.hpp for every file they answer; the rest is DEFERRED to the host reader.
//
// Two bodies.  read_scan_body, one wave per file: the header, then the directory 64 slots at a time -- a lane reads its 28-byte big-endian
// record byte by byte (the record sits at any address), matches it against the nine keys readab uses, a ballot per key finds the slot and
// counts repeats, bcast hands its fields to the wave.  What readab does with a slot, restated:
//     PCON's element type is forced to 1; a slot whose type is not 1, 2 or 4 is skipped; PBAS.2 / P2BA.1 / FWO_.1 are read under type 2,
//     PLOC.2 / DATA.9-12 under type 4, PCON.2 under type 1 -- a wanted name under another type is ignored
//     begin = dsize > 4 ? the slot's offset field : the address of that field (by dsize, not by count * esize)
//     a character payload is count + 1 bytes long, clipped at the end of the file; the extra byte counts in the common length
//     n = min(|PBAS|, |P2BA| unless that is empty, count of PCON, count of PLOC); channel i of DATA.9-12 is the letter FWO_.1[i]
// The conditions under which a file is answered are in include/tracy_hip.h; on top of them 8 * nsamples <= file_len (four channels that
// do not overlap: the promise of tracyhip_read_bound).  The wave writes a ReadDesc: status, format, sizes and where each payload begins.
// For SCF with 16-bit results the scan integrates every channel once without storing it: a value outside int16 defers the file before any
// of its samples is written.
//
// read_emit_body, one wave per (file, tile).  Tile 0 of a file writes the calls (positions, letters through the only_dna map, qualities);
// the tiles behind it belong to the four channels.  A lane owns one GROUP of kReadGroup samples, and groups are counted from the 8-element
// boundary below the channel's first OUTPUT element, so every whole group leaves as full-width stores whatever sample_offset and nsamples
// are; its 16 source bytes sit at any address (file_offset + begin is arbitrary, odd included) and are cut out of the aligned dwords that
// hold them (v_alignbyte), their halves swapped by one v_perm.  The two groups at a channel's ends go element by element.  An SCF channel
// is walked by ONE wave, kReadScfTile samples a step: the two running sums of the second differences are wave scans whose 16-bit carry
// passes from step to step,
//     v[k] = raw[k] + wrap16(raw[0] + .. + raw[k-1]),   w[k] = v[k] + wrap16(v[0] + .. + v[k-1])
// (trace_io.hpp:205-216: the carry wraps, the value does not).  Every output element is written exactly once, nothing outside
// [offset, offset + reported size).
//
// W: the wave concept of dev_wave.h (lane, ballot, bcast, sum, excl_sum).
#ifndef TRACY_AMD_READ_WAVE_H
#define TRACY_AMD_READ_WAVE_H

#include <cstdint>

#include "dp_lane.h"  // TR_HD

namespace tracyhip {

constexpr int32_t kReadStatusOk = 0, kReadStatusDeferred = 1, kReadStatusTooSmall = 2;  // TRACYHIP_READ_*
constexpr uint32_t kReadMaxCalls = 131071;        // the decompose limit, as basecalling
constexpr uint32_t kReadMinSamples = 3, kReadMaxSamples = 1u << 23;  // what tracyhip_basecall_traces answers
constexpr uint32_t kReadGroup = 8;                // samples per lane of an ABIF channel tile: 16 bytes in, 16 or 32 out
constexpr uint32_t kReadTile = 64 * kReadGroup;   // samples per tile
constexpr uint32_t kReadScfVec = 4;               // samples per lane and step of an SCF channel
constexpr uint32_t kReadScfTile = 64 * kReadScfVec;
constexpr uint32_t kReadAbsent = 0xffffffffu;     // ReadDesc::p2ba without a secondary

struct ReadFile {  // per file, built by the host from the job's and the result's HOST arrays
  uint64_t file_off;      // bytes
  uint64_t out_sig_off;   // elements
  uint64_t out_call_off;  // elements
  uint32_t file_len;
  uint32_t sample_cap, call_cap;
  uint32_t tile_first;         // of the emit launch's tiles; the file owns 1 + 4 * tiles_per_channel of them
  uint32_t tiles_per_channel;  // enough for any file of this length (read_channel_tiles)
  uint32_t unused;
};
struct ReadDesc {  // per file, written by the scan
  int32_t status, format;
  uint32_t nsamples, ncalls;
  uint32_t chan[4];  // where the samples of A, C, G, T begin, bytes from the file's start, as the four below
  uint32_t ploc, pbas, p2ba, pcon;
};
struct ReadArgs {
  const uint8_t* bytes;
  const ReadFile* fl;
  ReadDesc* desc;
  void* o_signal;  // payload results, each may be null
  int32_t* o_pos;
  uint8_t *o_b1, *o_b2, *o_qual;
  uint32_t ntraces, ntiles, sample_bytes;
};

// capacities that any answered file of this length fits: four channels take 8 bytes a sample, the positions 2 bytes a call
TR_HD uint32_t read_bound_samples(uint32_t file_len) { return file_len / 8 < kReadMaxSamples ? file_len / 8 : kReadMaxSamples; }
TR_HD uint32_t read_bound_calls(uint32_t file_len) { return file_len / 2 < kReadMaxCalls ? file_len / 2 : kReadMaxCalls; }
// groups are counted from the boundary below the first output element: one more than the samples fill, and one for the remainder
TR_HD uint32_t read_channel_tiles(uint32_t file_len) { return (read_bound_samples(file_len) / kReadGroup + 2 + 63) / 64; }

TR_HD int32_t read_be16(const uint8_t* p) { return (int16_t)(uint16_t)(((uint32_t)p[0] << 8) | p[1]); }
TR_HD int32_t read_be32(const uint8_t* p) {
  return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]);
}
TR_HD uint8_t read_only_dna(uint8_t c) { return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : (uint8_t)'N'; }  // replaceNonDna, abif.h:276-284
TR_HD int read_letter(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// the dword that begins r bytes into lo (then runs into hi), r in 1 .. 3
TR_HD uint32_t read_alignbyte(uint32_t hi, uint32_t lo, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * r));
#endif
}
// two big-endian 16-bit words as they lie in memory -> the same two words little-endian
TR_HD uint32_t read_swap16(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, x, 0x02030001u);
#else
  return ((x & 0x00ff00ffu) << 8) | ((x >> 8) & 0x00ff00ffu);
#endif
}
struct alignas(16) ReadQuad { uint32_t x, y, z, w; };
TR_HD uint32_t read_sext_lo(uint32_t x) { return (uint32_t)(int32_t)(int16_t)(uint16_t)x; }
TR_HD uint32_t read_sext_hi(uint32_t x) { return (uint32_t)((int32_t)x >> 16); }

// Group j of n big-endian 16-bit words at src (any address) to the elements of dst (the address of element 0; int32 with OUT32, else
// int16; aligned to its element).  A whole group is one (int16) or two (int32) 16-byte stores.
template <bool OUT32>
TR_HD void read_be16_group(const uint8_t* src, void* dst, uint32_t n, uint32_t j) {
  constexpr uint32_t SB = OUT32 ? 4 : 2;
  const uint32_t shift = (uint32_t)((reinterpret_cast<uintptr_t>(dst) / SB) % kReadGroup);
  const int64_t xlo = (int64_t)j * kReadGroup - shift;
  if (xlo >= (int64_t)n) return;
  if (xlo >= 0 && xlo + kReadGroup <= (int64_t)n) {
    const uint8_t* sp = src + 2 * xlo;
    const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(sp) & 3u);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sp - r);  // aligned dwords from the one that holds sp[0]
    uint32_t d0 = sw[0], d1 = sw[1], d2 = sw[2], d3 = sw[3];
    if (r) {  // (then sw[4] holds bytes of the group: an aligned dword that overlaps the caller's buffer is inside its allocation)
      const uint32_t d4 = sw[4];
      d0 = read_alignbyte(d1, d0, r); d1 = read_alignbyte(d2, d1, r); d2 = read_alignbyte(d3, d2, r); d3 = read_alignbyte(d4, d3, r);
    }
    d0 = read_swap16(d0); d1 = read_swap16(d1); d2 = read_swap16(d2); d3 = read_swap16(d3);
    if (OUT32) {
      ReadQuad* q = reinterpret_cast<ReadQuad*>(static_cast<int32_t*>(dst) + xlo);
      q[0] = ReadQuad{read_sext_lo(d0), read_sext_hi(d0), read_sext_lo(d1), read_sext_hi(d1)};
      q[1] = ReadQuad{read_sext_lo(d2), read_sext_hi(d2), read_sext_lo(d3), read_sext_hi(d3)};
    } else {
      *reinterpret_cast<ReadQuad*>(static_cast<int16_t*>(dst) + xlo) = ReadQuad{d0, d1, d2, d3};
    }
    return;
  }
  const uint32_t x0 = xlo < 0 ? 0u : (uint32_t)xlo;
  const uint32_t x1 = xlo + kReadGroup < (int64_t)n ? (uint32_t)(xlo + kReadGroup) : n;
  for (uint32_t x = x0; x < x1; ++x) {
    const int32_t v = read_be16(src + 2 * (uint64_t)x);
    if (OUT32) static_cast<int32_t*>(dst)[x] = v;
    else static_cast<int16_t*>(dst)[x] = (int16_t)v;
  }
}

// One SCF channel of ns second differences at src, integrated twice; sink(x, w[x]) is called once for every sample by the lane that owns it.
// Every lane of the wave calls this.
template <class W, class Sink>
TR_HD void read_scf_channel(W& w, const uint8_t* src, uint32_t ns, Sink&& sink) {
  uint32_t carry1 = 0, carry2 = 0;  // the sums of raw / of v over the steps before (only their low 16 bits are ever used)
  for (uint32_t base = 0; base < ns; base += kReadScfTile) {
    const uint32_t x0 = base + w.lane() * kReadScfVec;
    int32_t r[kReadScfVec];
    uint32_t s = 0;
#pragma unroll
    for (uint32_t i = 0; i < kReadScfVec; ++i) {
      r[i] = x0 + i < ns ? read_be16(src + 2 * (uint64_t)(x0 + i)) : 0;
      s += (uint32_t)r[i];
    }
    uint32_t p1 = w.excl_sum(s) + carry1;
    carry1 += w.sum(s);
    int32_t v[kReadScfVec];
    uint32_t s2 = 0;
#pragma unroll
    for (uint32_t i = 0; i < kReadScfVec; ++i) {
      v[i] = x0 + i < ns ? r[i] + (int32_t)(int16_t)(uint16_t)p1 : 0;
      p1 += (uint32_t)r[i];
      s2 += (uint32_t)v[i];
    }
    uint32_t p2 = w.excl_sum(s2) + carry2;
    carry2 += w.sum(s2);
#pragma unroll
    for (uint32_t i = 0; i < kReadScfVec; ++i) {
      if (x0 + i < ns) sink(x0 + i, v[i] + (int32_t)(int16_t)(uint16_t)p2);
      p2 += (uint32_t)v[i];
    }
  }
}

// the nine keys of readab: 0 PBAS.2, 1 P2BA.1, 2 FWO_.1, 3 PLOC.2, 4 .. 7 DATA.9 .. 12, 8 PCON.2; -1: another slot
constexpr int kReadKeys = 9;
TR_HD uint32_t read_name(char a, char b, char c, char d) { return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint8_t)d; }
TR_HD int read_key(uint32_t name, int32_t number) {
  if (name == read_name('P', 'B', 'A', 'S')) return number == 2 ? 0 : -1;
  if (name == read_name('P', '2', 'B', 'A')) return number == 1 ? 1 : -1;
  if (name == read_name('F', 'W', 'O', '_')) return number == 1 ? 2 : -1;
  if (name == read_name('P', 'L', 'O', 'C')) return number == 2 ? 3 : -1;
  if (name == read_name('D', 'A', 'T', 'A')) return number >= 9 && number <= 12 ? number - 5 : -1;
  if (name == read_name('P', 'C', 'O', 'N')) return number == 2 ? 8 : -1;
  return -1;
}
TR_HD int32_t read_key_type(int key) { return key <= 2 ? 2 : key <= 7 ? 4 : 1; }   // the element type a key is read under
TR_HD int32_t read_key_esize(int key) { return key >= 3 && key <= 7 ? 2 : 1; }     // its natural element size

struct ReadTag {
  uint32_t found;  // slots that name the key under the type it is read under
  int32_t count, esize;
  int64_t begin;
};

// false: not a file the device answers.  Every lane of the wave calls this with the same arguments.
template <class W>
TR_HD bool read_scan_abif(W& w, const uint8_t* p, uint64_t flen, ReadDesc& d) {
  if (flen < 34) return false;
  const int32_t slot = read_be16(p + 16), nslots = read_be32(p + 18), dir = read_be32(p + 26);
  if (slot != 28 || nslots <= 0 || dir < 0 || (uint64_t)dir + 28ull * (uint32_t)nslots > flen) return false;
  ReadTag tag[kReadKeys];
#pragma unroll
  for (int k = 0; k < kReadKeys; ++k) tag[k] = ReadTag{0, 0, 0, 0};
  for (uint32_t base = 0; base < (uint32_t)nslots; base += 64) {
    const uint32_t i = base + w.lane();
    int key = -1;
    int32_t count = 0, esize = 0;
    int64_t begin = 0;
    if (i < (uint32_t)nslots) {
      const uint64_t at = (uint64_t)dir + 28ull * i;
      const uint8_t* e = p + at;
      key = read_key((uint32_t)read_be32(e), read_be32(e + 4));
      int32_t etype = read_be16(e + 8);
      if (key == 8) etype = 1;
      if (key >= 0 && etype != read_key_type(key)) key = -1;
      esize = read_be16(e + 10);
      count = read_be32(e + 12);
      begin = read_be32(e + 16) > 4 ? (int64_t)read_be32(e + 20) : (int64_t)at + 20;
    }
#pragma unroll
    for (int k = 0; k < kReadKeys; ++k) {
      const uint64_t m = w.ballot(key == k);
      if (!m) continue;  // (the same in every lane)
      const uint32_t from = (uint32_t)__builtin_ctzll(m);
      tag[k].found += (uint32_t)__builtin_popcountll(m);
      tag[k].count = (int32_t)w.bcast((uint32_t)count, from);
      tag[k].esize = (int32_t)w.bcast((uint32_t)esize, from);
      const uint32_t lo = w.bcast((uint32_t)(uint64_t)begin, from), hi = w.bcast((uint32_t)((uint64_t)begin >> 32), from);
      tag[k].begin = (int64_t)(((uint64_t)hi << 32) | lo);
    }
  }
  uint64_t len[kReadKeys];  // bytes readab takes: count * esize, one more for the character payloads where the file has it
#pragma unroll
  for (int k = 0; k < kReadKeys; ++k) {
    len[k] = 0;
    const ReadTag& g = tag[k];
    if (g.found > 1 || (g.found == 0 && k != 1)) return false;
    if (g.found == 0) continue;
    if (g.esize != read_key_esize(k) || g.count < 0 || g.begin < 0) return false;
    const uint64_t bytes = (uint64_t)g.count * (uint32_t)g.esize;
    if ((uint64_t)g.begin > flen || bytes > flen - (uint64_t)g.begin) return false;
    len[k] = bytes + ((k <= 2 && (uint64_t)g.begin + bytes < flen) ? 1 : 0);
  }
  if (len[2] < 4) return false;
  uint32_t seen = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = read_letter(p[tag[2].begin + i]);
    if (k < 0 || (seen >> k & 1u)) return false;
    seen |= 1u << k;
    d.chan[k] = (uint32_t)tag[4 + i].begin;
  }
  const int32_t ns = tag[4].count;
  if (tag[5].count != ns || tag[6].count != ns || tag[7].count != ns) return false;
  if (ns < (int32_t)kReadMinSamples || ns > (int32_t)kReadMaxSamples || 8ull * (uint32_t)ns > flen) return false;
  const bool second = tag[1].found == 1 && len[1] > 0;  // (an empty P2BA is readab's "absent")
  uint64_t n = len[0];
  if (second && len[1] < n) n = len[1];
  if ((uint64_t)tag[8].count < n) n = (uint64_t)tag[8].count;
  if ((uint64_t)tag[3].count < n) n = (uint64_t)tag[3].count;
  if (n < 1 || n > kReadMaxCalls) return false;
  d.nsamples = (uint32_t)ns;
  d.ncalls = (uint32_t)n;
  d.ploc = (uint32_t)tag[3].begin; d.pbas = (uint32_t)tag[0].begin; d.pcon = (uint32_t)tag[8].begin;
  d.p2ba = second ? (uint32_t)tag[1].begin : kReadAbsent;
  return true;
}

template <class W>
TR_HD bool read_scan_scf(W& w, const uint8_t* p, uint64_t flen, uint32_t sample_bytes, ReadDesc& d) {
  if (flen < 40) return false;
  const int32_t samples = read_be32(p + 4), samples_at = read_be32(p + 8), bases = read_be32(p + 12), bases_at = read_be32(p + 24);
  const uint8_t* v = p + 36;
  auto digit = [](uint8_t c) { return c >= '0' && c <= '9'; };
  if (!(v[0] >= '3' && v[0] <= '9' && v[1] == '.' && digit(v[2]) && digit(v[3]))) return false;
  if (samples < (int32_t)kReadMinSamples || samples > (int32_t)kReadMaxSamples || bases < 1 || bases > (int32_t)kReadMaxCalls) return false;
  if (samples_at < 0 || bases_at < 0) return false;
  if ((uint64_t)samples_at > flen || 8ull * (uint32_t)samples > flen - (uint64_t)samples_at) return false;
  if ((uint64_t)bases_at > flen || 4ull * (uint32_t)bases > flen - (uint64_t)bases_at) return false;
  for (uint32_t k = 0; k < 4; ++k) d.chan[k] = (uint32_t)samples_at + 2u * k * (uint32_t)samples;
  if (sample_bytes == 2) {  // every integrated sample fits int16, known before one is written
    bool wide = false;
    for (uint32_t k = 0; k < 4; ++k)
      read_scf_channel(w, p + d.chan[k], (uint32_t)samples, [&](uint32_t, int32_t x) { wide = wide || x < -32768 || x > 32767; });
    if (w.ballot(wide)) return false;
  }
  d.nsamples = (uint32_t)samples;
  d.ncalls = (uint32_t)bases;
  d.ploc = (uint32_t)bases_at;
  d.pbas = d.pcon = 0;
  d.p2ba = kReadAbsent;
  return true;
}

// file t of the launch: format, the conditions, the sizes against the capacities; the descriptor
template <class W>
TR_HD void read_scan_body(W& w, const ReadArgs& a, uint32_t t) {
  const ReadFile& f = a.fl[t];
  const uint8_t* p = a.bytes + f.file_off;
  const uint64_t flen = f.file_len;
  ReadDesc d{};
  d.status = kReadStatusDeferred;
  d.format = -1;  // traceFormat, scf.h:18-34
  if (flen >= 4) {
    const uint32_t magic = (uint32_t)read_be32(p);
    d.format = magic == read_name('A', 'B', 'I', 'F') ? 0 : magic == read_name('.', 's', 'c', 'f') ? 1 : -1;
  }
  bool ok = false;
  if (d.format == 0) ok = read_scan_abif(w, p, flen, d);
  else if (d.format == 1) ok = read_scan_scf(w, p, flen, a.sample_bytes, d);
  if (ok) {
    const bool calls = a.o_pos || a.o_b1 || a.o_b2 || a.o_qual;
    d.status = ((a.o_signal && d.nsamples > f.sample_cap) || (calls && d.ncalls > f.call_cap)) ? kReadStatusTooSmall : kReadStatusOk;
  } else {
    const int32_t format = d.format;
    d = ReadDesc{};
    d.status = kReadStatusDeferred;
    d.format = format;
  }
  if (w.lane() == 0) a.desc[t] = d;
}

// the file that owns tile `tile`: the last one whose tile_first is <= tile (every file owns a tile: tile_first rises)
TR_HD uint32_t read_owner(const ReadFile* fl, uint32_t ntraces, uint32_t tile) {
  uint32_t lo = 0, hi = ntraces;  // first file whose tile_first is > tile
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (fl[mid].tile_first <= tile) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

template <bool S16, class W>
TR_HD void read_emit_body(W& w, const ReadArgs& a, uint32_t tile) {
  const uint32_t t = read_owner(a.fl, a.ntraces, tile);
  const ReadFile& f = a.fl[t];
  const ReadDesc d = a.desc[t];
  if (d.status != kReadStatusOk) return;  // (the whole wave)
  const uint8_t* p = a.bytes + f.file_off;
  const uint32_t q = tile - f.tile_first, lane = w.lane(), ns = d.nsamples, n = d.ncalls;
  const bool abif = d.format == 0;
  if (q == 0) {  // the calls
    if (a.o_pos) {
      int32_t* o = a.o_pos + f.out_call_off;
      if (abif) {
        for (uint32_t j = lane; j < n / kReadGroup + 2; j += 64) read_be16_group<true>(p + d.ploc, o, n, j);
      } else {
        for (uint32_t c = lane; c < n; c += 64) o[c] = read_be32(p + d.ploc + 4ull * c);
      }
    }
    for (uint32_t c = lane; c < n; c += 64) {
      if (a.o_b1) a.o_b1[f.out_call_off + c] = abif ? read_only_dna(p[d.pbas + c]) : (uint8_t)0;
      if (a.o_b2) a.o_b2[f.out_call_off + c] = (abif && d.p2ba != kReadAbsent) ? read_only_dna(p[d.p2ba + c]) : (uint8_t)0;
      if (a.o_qual) a.o_qual[f.out_call_off + c] = abif ? p[d.pcon + c] : (uint8_t)0;
    }
    return;
  }
  if (!a.o_signal) return;
  const uint32_t k = (q - 1) / f.tiles_per_channel, tic = (q - 1) % f.tiles_per_channel;
  if (k >= 4) return;
  const uint64_t at = f.out_sig_off + (uint64_t)k * ns;
  if (abif) {
    void* dst = S16 ? static_cast<void*>(static_cast<int16_t*>(a.o_signal) + at) : static_cast<void*>(static_cast<int32_t*>(a.o_signal) + at);
    read_be16_group<!S16>(p + d.chan[k], dst, ns, tic * 64 + lane);
  } else if (tic == 0) {
    if (S16) {
      int16_t* o = static_cast<int16_t*>(a.o_signal) + at;
      read_scf_channel(w, p + d.chan[k], ns, [&](uint32_t x, int32_t v) { o[x] = (int16_t)v; });
    } else {
      int32_t* o = static_cast<int32_t*>(a.o_signal) + at;
      read_scf_channel(w, p + d.chan[k], ns, [&](uint32_t x, int32_t v) { o[x] = v; });
    }
  }
}

}  // namespace tracyhip
#endif
