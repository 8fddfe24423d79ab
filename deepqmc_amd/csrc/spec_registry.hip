// spec_registry.hip -- the plan-specialised sub-step kernels linked into this library (csrc/gen/*.hip, written by
// deepqmc_amd/codegen) and the host-side packer of their weight tapes.
#include "spec_device.h"

#include <cstring>

namespace dqmc {

#define DQMC_SPEC_KERNEL(name) const SpecKernel* spec_kernel_##name();
#include "gen/spec_list.inc"
#undef DQMC_SPEC_KERNEL

typedef const SpecKernel* (*SpecGetter)();
static const SpecGetter kSpecKernels[] = {
#define DQMC_SPEC_KERNEL(name) &spec_kernel_##name,
#include "gen/spec_list.inc"
#undef DQMC_SPEC_KERNEL
    nullptr};

const SpecKernel* find_spec_kernel(uint64_t hash) {
  for (const SpecGetter* k = kSpecKernels; *k; ++k) {
    const SpecKernel* sk = (*k)();
    if (sk->hash == hash) return sk;
  }
  return nullptr;
}

// piece pl (0..2) of the three-bf16 split of a float (round to nearest even, exact residuals: common.h bf_split8)
static uint16_t bf16_piece(float v, int pl) {
  auto rne = [](float f) -> uint16_t {
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  };
  auto up = [](uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
  uint16_t h = rne(v);
  for (int k = 0; k < pl; ++k) { v = v - up(h); h = rne(v); }
  return h;
}

// The layout of the tape, once: the fragments in consumption order (SpecTapeEntry), zero padded to whole ring stages.
// bf(word index, flat weight entry of the low half or -1, of the high half or -1, plane, scale) and plain(word index, entry
// or -1, scale) are called for every word of every fragment; the words of the padding are never visited.
template <typename Bf, typename Plain>
static void spec_walk_tape(const SpecKernel& k, Bf&& bf, Plain&& plain) {
  size_t frag = 0;
  for (int e = 0; e < k.n_entries; ++e) {
    const SpecTapeEntry& t = k.entries[e];
    const int32_t* map = k.maps + t.map;
    if (t.kind == 0) {
      for (int pl = 0; pl < 3; ++pl) {
        const size_t f = (frag + pl) * 256;
        for (int lane = 0; lane < 64; ++lane) {
          const int c = lane & 15, g = lane >> 4;
          for (int j = 0; j < 4; ++j) {
            long src[2];
            for (int h = 0; h < 2; ++h) {
              const int row = map[8 * g + 2 * j + h];
              src[h] = (row >= 0 && c < t.ncol) ? (long)t.w_off + (long)row * t.ldw + t.col0 + c : -1;
            }
            bf(f + lane * 4 + j, src[0], src[1], pl, t.scale);
          }
        }
      }
      frag += 3;
    } else {
      for (int q = 0; q < 256; ++q) plain(frag * 256 + q, (long)map[q], t.scale);
      frag += 1;
    }
  }
}

void spec_pack_tape(const SpecKernel& k, const float* w, uint32_t* tape) {
  memset(tape, 0, (size_t)k.tape_bytes);
  spec_walk_tape(
      k,
      [&](size_t at, long s0, long s1, int pl, float scale) {
        const float v0 = s0 >= 0 ? w[s0] * scale : 0.0f, v1 = s1 >= 0 ? w[s1] * scale : 0.0f;
        tape[at] = (uint32_t)bf16_piece(v0, pl) | (uint32_t)bf16_piece(v1, pl) << 16;
      },
      [&](size_t at, long s, float scale) {
        const float v = s >= 0 ? w[s] * scale : 0.0f;
        memcpy(tape + at, &v, 4);
      });
}

void spec_tape_sources(const SpecKernel& k, PackSrc* out) {
  const size_t n = (size_t)k.tape_bytes / 4;
  for (size_t q = 0; q < n; ++q) out[q] = PackSrc{-1, -1, 1.0f, -1};      // (padding: plain zero words)
  spec_walk_tape(
      k, [&](size_t at, long s0, long s1, int pl, float scale) { out[at] = PackSrc{(int32_t)s0, (int32_t)s1, scale, pl}; },
      [&](size_t at, long s, float scale) { out[at] = PackSrc{(int32_t)(s >= 0 ? s : -1), -1, scale, -1}; });
}

}  // namespace dqmc
