// SignalConv2D, third-generation bfloat16 implicit-GEMM kernel (conv3_bf16_kernel) and its host side, run_conv3:
// route_gemm (signal_conv.hip) tries it first.
#include "conv_shared.h"

namespace tfc {

// Third-generation kernel: a workgroup computes an 8 x 32 block of low-resolution output pixels of ONE image
// from an input patch staged in LDS one 16-channel block at a time.
struct Conv3Geom {
  int BXn, BYn;            // blocks per image row / column
  int PW, PWh;             // patch columns; columns per x-parity plane (ceil(PW / sd))
  int lg;                  // log2(sd), sd in {1, 2}
  int granules;            // 16-byte granules of a patch: PH * sd * 2 * PWh, order [row][x parity][h][x / sd]
  int pixels;              // PH * PW
  int gcount;              // column groups this launch covers ...
  int glist[kMaxGroups];   // ... and which
  int ostage;              // byte offset in LDS of the epilogue's staging area (4 waves x 8 KB), see the kernel
  int obias;               // ... and of the bias (Cout floats, parked by the prologue)
  int oimage;              // GDN as the activation: where gamma's fragment image lives in LDS
  unsigned int bx_mul, bx_sh, by_mul, by_sh, gc_mul, gc_sh, pw_mul, pw_sh;   // fast_div by BXn, BYn, gcount, PW
};

// Workgroup -> work item, XCD-aware.  The dispatcher hands consecutive workgroup ids to the 8 XCDs in turn, each with
// its own L2: with work item = workgroup id, neighbouring blocks of an image — which read the same halo rows — run on
// different XCDs and each fetches its own copy.  xcd_order gives XCD x the x-th contiguous eighth of the items instead
// (a bijection for any count), so the blocks an XCD runs at one time are neighbours.  `on` = 0: the identity.
// Measured at the C4 shapes (same box, alternating): the third-generation kernel's transposed layers 8.05-8.14 -> 7.92-7.96
// ms (192x128 input) and 0.64 -> 0.61 ms (48x32); the second-generation stride-2 layers 6.79 -> 6.96 ms: only the third
// generation uses it.
constexpr unsigned int kXcds = 8;
__device__ inline unsigned int xcd_order(unsigned int id, unsigned int count, int on) {
  if (!on || count < 2 * kXcds) return id;
  const unsigned int x = id % kXcds, k = id / kXcds;
  const unsigned int per = count / kXcds, extra = count % kXcds;
  return x * per + (x < extra ? x : extra) + k;
}

// ---------------------------------------------------------------------------
// bf16 main kernel, third generation (5x5 / 3x3 layers between wide feature maps: Cin % 16 == 0,
// Cout = 128 or 192 per group).  What the second generation spends beside its MFMAs is the B operand: a
// 16-byte gather per lane, tap and K step straight from the NHWC tensor (every input value requested kh*kw/sd^2
// times), each with its bounds test, address select and tap walk.  Here a workgroup owns an 8 x 32 block of
// low-resolution output pixels of one image and
//   * stages the input PATCH of that block in LDS, one 16-channel block at a time, double-buffered: every input
//     value is requested once per workgroup (+ the halo), bounds are tested once per granule and channel block
//     by the loader, and out-of-image positions are zeros in LDS;
//   * runs K channel block by channel block, the taps inside: a tap is a wave-uniform LDS offset, so a B
//     fragment is one ds_read_b128 at (per-lane base) + (scalar tap offset) — no per-lane arithmetic;
//   * lays the patch out as [row][x parity][h][x / sd] granules of 16 bytes (h = which 8 of the 16 channels):
//     the 32 pixels of a tile (one output row segment, input stride sd) are consecutive granules of one
//     parity / h plane, i.e. all 64 banks once per 16-lane group of the ds_read_b128;
//   * keeps of the second generation: weights as packed A fragments in a double-buffered LDS chunk (here CH K steps =
//     CH taps of one channel block, CH | taps), A / B fragments double-buffered in registers, 2 pixel tiles x TILES
//     column tiles per wave.
// NPG = 16-byte patch pieces per thread (granules / 256, rounded up).
// Round 6 (measured from the inside with the timing build below; DESIGN.md §3, profiles/r06_notes.md):
//   * the patch loader reads a pixel's 32 bytes of the channel block with a lane PAIR (32 lines per request instead of 64);
//   * the weight chunks go global -> LDS by buffer_load ... lds (WDMA), not through registers;
//   * every staging instruction sits behind an MFMA of its own (slots, below);
//   * the output leaves as whole 128-byte lines through a wave-private LDS area, non-temporal for big outputs;
//   * GDN / IGDN as the activation: builds of their own (GDNK), no scratch.
//   * one ITEM per workgroup: a block and one of the launch's column groups (round 6; before: a workgroup took a
//     block's groups, or every W-th block, one after the other with the next item's first requests under the last K
//     steps — per item the same time, tools/conv3_clock_probe.py: what the prologue saved the longer K loop and the
//     bookkeeping between items took, and it kept ~90 registers of next-item state alive through the epilogue);
//   * the K steps of a channel block are unrolled into ONE basic block (template NCH chunks x CH K steps): taps are
//     compile-time indexes into a table of scalar offsets, and the staging of a chunk boundary sits between the MFMAs.
// TFC_CONV3_EXP (build switch, timing experiments only — results are wrong): 1 no barriers, 2 no weight staging,
// 4 no patch staging, 32 no output stores (tools/conv3_variants.sh).
// ---------------------------------------------------------------------------
#ifndef TFC_CONV3_EXP
#define TFC_CONV3_EXP 0
#endif
#if TFC_CONV3_EXP & 64
// timing builds only (tools/conv3_clock_probe.py): per workgroup (the first kConv3ClockWgs of a launch) the 100 MHz
// clock at entry, behind the prologue's barrier, at the end of the K loop, with the stores issued, and with them
// acknowledged; [5] = the CU (XCC, SE, CU id) it ran on
constexpr int kConv3ClockWgs = 16384;
__device__ unsigned long long g_conv3_clocks[kConv3ClockWgs * 8];
// ... and core-clock cycles its first wave waited in the K loop: [ch] for the weight chunk stored at the start of chunk ch of
// a channel block (ch < 5), [5] at the barriers, [6] the K loop, [7] for the LDS reads in front of the MFMAs of a K step
__device__ unsigned long long g_conv3_waits[kConv3ClockWgs * 8];
// (timing build: the cycles a staging instruction takes to ISSUE — the wave issues in order, the matrix pipe has nothing
// to start while it does — summed per kind in kwait[kind]: 0 weight requests, 1 patch requests, 2 / 3 their LDS writes)
#define TFC_CONV3_ISSUE(kind, stmt)                       \
  do {                                                    \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    \
    const long long i0__ = __builtin_readcyclecounter();  \
    stmt;                                                 \
    const long long i1__ = __builtin_readcyclecounter();  \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    \
    kwait[kind] += i1__ - i0__;                           \
  } while (0)
#define TFC_CONV3_CLOCK(slot)                                                                              \
  do {                                                                                                     \
    if (threadIdx.x == 0 && blockIdx.x < kConv3ClockWgs) g_conv3_clocks[blockIdx.x * 8 + (slot)] = wall_clock64(); \
  } while (0)
#else
#define TFC_CONV3_ISSUE(kind, stmt) stmt
#define TFC_CONV3_CLOCK(slot) do {} while (0)
#endif
// workgroup barrier that orders LDS traffic only (a __syncthreads also waits for the global loads in flight)
#define TFC_LDS_BARRIER()                                                \
  do {                                                                   \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");      \
    __builtin_amdgcn_s_barrier();                                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");      \
  } while (0)
// OUTF32 (round 6): the float32 accumulators + bias leave as float32 (the float32 layers that run as six bfloat16
// planes, conv_split_x_kernel).
template <int TILES, int CH, int NCH, int NPG, int GDNK = 0, bool OUTF32 = false>
__global__ void __launch_bounds__(256, 1) conv3_bf16_kernel(const __bf16* x, const void* packed,
                                                            const float* bias, __bf16* y, ConvGeom c,
                                                            Conv3Geom d) {
  extern __shared__ unsigned char smem[];          // 2 patches of PATCH_BYTES | 2 weight chunks of STAGE * 4 KB
  // GDNK: 0 none, 1 GDN (y / norm), 2 IGDN (y * norm) as the activation.  A build each — ONE straight-line epilogue: with
  // the two as branches of one build the compiler hoisted what they share (every y word split into its two floats, 192
  // registers) in front of the branch, and the epilogue ran out of scratch (12 us per item instead of 5)
  constexpr bool GDN = GDNK != 0;
  // MT = 2 pixel tiles per wave: four waves, one per SIMD.  (Round 6, measured and not kept: MT = 1 with EIGHT waves, two
  // per SIMD at <= 220 registers, so that one wave's MFMAs run while the other issues its staging instructions — the
  // stride-2 5x5 layer took 5.68 ms against 5.64: the second wave of a SIMD does not fill those gaps, profiles/r06_notes.md)
  constexpr int MT = 2;
  constexpr int NTHR = 256;
  constexpr unsigned int TPIECE = NTHR * 16u;                // bytes of one 16-byte piece per thread
  constexpr int CHUNK_FRAGS = CH * TILES * 64;
  constexpr int STAGE = (CHUNK_FRAGS + NTHR - 1) / NTHR;    // 16-byte pieces per thread and weight chunk
  // a patch buffer: the granules + room for the (unread) granules of threads past the patch's last pixel
  constexpr unsigned int PATCH_BYTES = NPG * 4096u + (NPG > 4 ? 2048u : 0u);
  constexpr int NPT = NPG;
  constexpr unsigned int WBUF_BYTES = STAGE * TPIECE;
  static_assert(NPG % 2 == 0, "two pieces per patch pixel");
  // WDMA (round 6): the weight chunks travel global -> LDS without passing the wave's registers (buffer_load ... lds: a
  // wave's piece is 1 KB contiguous on both sides; no ds_write_b128, 37 cycles of issue each, and 32 registers less).
  // Short chunks (3 / 4 K steps): chunk c + 2 is requested in the LAST K step of chunk c — behind the barrier that ended the
  // reads of chunk c's own buffer, which it goes to — and has to have landed at chunk c + 1's barrier: CH K steps.  The
  // 5-K-step chunks: chunk c + 1 in the FIRST K step of chunk c (CH - 1 K steps; measured against the last K step of the chunk
  // before on the stride-2 5x5 layer: 5.11 / 5.18 ms, through registers 5.22; the transposed layer's three launches 5.68
  // against 5.75).  TFC_CONV3_WDMA = 0: through registers (requested a chunk earlier).
#ifndef TFC_CONV3_WDMA
#define TFC_CONV3_WDMA 1
#endif
  constexpr bool WDMA = TFC_CONV3_WDMA != 0;
  constexpr bool WEARLY = CH == 5;            // (see above) request in K step 0 of the chunk before, else K step CH - 1 of two before
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6, h = lane >> 5, l = lane & 31;
  const int wave_u = __builtin_amdgcn_readfirstlane(wid);
  const int lg = d.lg, sd = 1 << lg, PWh = d.PWh;
  const int cb = c.Cin / 16;
  unsigned char* wl = smem + 2 * PATCH_BYTES;

  // ---- the workgroup's ITEM: (block u / gcount, group glist[u % gcount]) for workgroup u in XCD order (the groups
  // of a block, and neighbouring blocks, meet in one L2) ----
  const unsigned int u = xcd_order(blockIdx.x, gridDim.x, c.xcd);
  TFC_CONV3_CLOCK(0);
#if TFC_CONV3_EXP & 64
  if (threadIdx.x == 0 && blockIdx.x < kConv3ClockWgs) {
    unsigned int hwid, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_conv3_clocks[blockIdx.x * 8 + 5] = (static_cast<unsigned long long>(xcc & 0xF) << 32) | hwid;
  }
#endif

  struct Item {                  // wave-uniform
    long long n;
    int qx0, qy0, group;
    int uy0, uy1, ux0, ux1;
  };
  // (divisions as multiplications, fast_div: a 64-bit division is a ~150-instruction loop in front of the first request)
  auto item_at = [&](unsigned int t) -> Item {
    Item it;
    const unsigned int blk = fast_div(t, d.gc_mul, d.gc_sh);
    it.group = d.glist[t - blk * d.gcount];
    const unsigned int row = fast_div(blk, d.bx_mul, d.bx_sh);          // n * BYn + by
    const unsigned int img = fast_div(row, d.by_mul, d.by_sh);
    it.qx0 = static_cast<int>(blk - row * d.BXn) * 32;
    it.qy0 = static_cast<int>(row - img * d.BYn) * 8;
    it.n = img;
    it.uy0 = c.ty0[it.group]; it.uy1 = c.ty1[it.group]; it.ux0 = c.tx0[it.group]; it.ux1 = c.tx1[it.group];
    return it;
  };

  // ---- patch loader.  Piece j of a thread = half tid & 1 (8 of the 16 channels) of patch pixel j * 128 + tid / 2: a
  // lane PAIR reads the 32 contiguous bytes a pixel has of the channel block, an instruction 32 pixels.  (Round 6;
  // before, a thread read both halves of pixel j * 256 + tid with two instructions of 64 pixels each: the CU's address
  // unit takes ~4 cycles per 128-byte line an instruction touches — 250 cycles measured for one of those, 13 for a
  // request of 1 KB contiguous, tools/conv3_clock_probe.py — and with 64 lines each the patch requests of the four waves
  // kept it busy 390 cycles of a K step's 650: half the lines per instruction, the same number of instructions.)
  // The granule a piece goes to is the same for every item, the place it comes from (poff) is per item.  Buffer loads:
  // a pixel outside the image has an offset outside the image's buffer and reads as zeros ----
  unsigned int pdst[NPT];                 // granule of (pixel, h = tid & 1)
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const int q = j * (NTHR / 2) + (tid >> 1);
    const int py = fast_div(q, d.pw_mul, d.pw_sh), px = q - py * d.PW;
    // (pixels past the patch: a granule behind it, inside the padded buffer, that nobody reads)
    pdst[j] = q < d.pixels ? static_cast<unsigned int>(((((py << lg) + (px & (sd - 1))) * 2 + (tid & 1)) * PWh + (px >> lg)) * 16)
                           : PATCH_BYTES - 16u * PWh - 16u;
  }
  auto patch_offsets = [&](int qx0, int qy0, unsigned int* poff) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int q = j * (NTHR / 2) + (tid >> 1);
      const int py = fast_div(q, d.pw_mul, d.pw_sh), px = q - py * d.PW;
      const int iy = qy0 * sd - c.py0 + py, ix = qx0 * sd - c.px0 + px;
      const bool ok = (q < d.pixels) & (static_cast<unsigned int>(iy) < static_cast<unsigned int>(c.H)) &
                      (static_cast<unsigned int>(ix) < static_cast<unsigned int>(c.W));
      poff[j] = ok ? static_cast<unsigned int>((iy * c.W + ix) * c.Cin * 2 + 16 * (tid & 1)) : 0x80000000u;
    }
  };
  auto image_rsrc = [&](long long n) -> __amdgpu_buffer_rsrc_t {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(x + n * c.H * c.W * c.Cin), 0,
                                             c.H * c.W * c.Cin * 2, 0x00020000);
  };
  u32x4 pst[NPT];
  auto pfetch = [&](__amdgpu_buffer_rsrc_t xr, const unsigned int* poff, int cbi) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NPT; ++j) pst[j] = __builtin_amdgcn_raw_buffer_load_b128(xr, poff[j], cbi * 32, 0);
  };
  auto pstore = [&](int buf) __attribute__((always_inline)) {
    unsigned char* dst = smem + buf * PATCH_BYTES;
#pragma unroll
    for (int j = 0; j < NPT; ++j) *reinterpret_cast<u32x4*>(dst + pdst[j]) = pst[j];
  };

  // ---- weights: the packed A fragments of a group, chunk by chunk; the request runs two chunks ahead of the K loop
  // (chunks past the group's end are outside the buffer: zeros, no traffic) ----
  auto weight_rsrc = [&](const Item& it) -> __amdgpu_buffer_rsrc_t {
    return __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(static_cast<const unsigned char*>(packed)) +
            static_cast<size_t>(it.group) * c.ksteps * TILES * 64 * 16,
        0, NCH * cb * (CHUNK_FRAGS * 16), 0x00020000);
  };
  u32x4 stage[STAGE];
  auto wfetch = [&](__amdgpu_buffer_rsrc_t r, int chunk) __attribute__((always_inline)) {
    const unsigned int v0 = static_cast<unsigned int>(chunk) * (CHUNK_FRAGS * 16u) + tid * 16u;
#pragma unroll
    for (int i = 0; i < STAGE; ++i) stage[i] = __builtin_amdgcn_raw_buffer_load_b128(r, v0 + i * TPIECE, 0, 0);
  };
  auto wstore = [&](int buf) __attribute__((always_inline)) {
    u32x4* dst = reinterpret_cast<u32x4*>(wl + buf * WBUF_BYTES) + tid;
#pragma unroll
    for (int i = 0; i < STAGE; ++i) dst[i * NTHR] = stage[i];
  };

  // ---- B: per-lane granule of (tile p, tap (0, 0)); a tap adds a wave-uniform offset ----
  unsigned int lb[MT];
#pragma unroll
  for (int p = 0; p < MT; ++p) {
    const int row = MT * wid + p;
    lb[p] = static_cast<unsigned int>(((row * sd * sd * 2 + h) * PWh + l) * 16);
  }
  auto tap_offset = [&](int uy, int ux) -> unsigned int {
    return static_cast<unsigned int>(((((uy << lg) + (ux & (sd - 1))) * 2) * PWh + (ux >> lg)) * 16);
  };

  f32x16 acc[MT][TILES];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < MT; ++p)
#pragma unroll
      for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][t][r] = 0.f;
  };
  zero_acc();

  // ---- epilogue of an item: acc[p][t][4q + r] = column group_base + 32t + 8q + 4h + r of pixel
  // (qy0 + MT wid + p, qx0 + l); 16-byte stores as in the second generation (Cout % 8 == 0) ----
  // ---- GDN / IGDN as the activation (GDN): the block's accumulators are all TILES * 32 channels of its pixels, in
  // the register layout the GDN kernel's B fragments have (gdn_common.h: K step s of a lane = channels 16 s + 4 h +
  // {0..3} and + 8), so |y| goes into the gamma contraction straight from the accumulators: 4 TILES^2 MFMAs per wave
  // against the K loop's thousands.  gamma's A fragments (the prepared image, 72 KB at 192 channels) are staged in LDS
  // over the two weight buffers — from L2 a K step of them is ~0.7 us away and 0.1 us of MFMAs (measured: +50 % on the
  // layer).  y is rounded to bfloat16 first: the same values the
  // unfused pair (convolution, then the GDN kernel on its output) works on, contracted in the same order ----
  constexpr int GDN_IMAGE_BYTES = TILES * 2 * TILES * 64 * 16 + TILES * 32 * 4;                   // fragments, beta
  constexpr int GDN_PIECES = (GDN_IMAGE_BYTES + static_cast<int>(TPIECE) - 1) / static_cast<int>(TPIECE);   // 16-byte pieces per thread
  // GRES: the transposed layers' builds (small patch, short weight chunks) have the LDS to keep the image for the whole
  // item — copied by the prologue beside the first patch and weight chunk, no barriers or copy in the stage: their items
  // are 4-9 taps long (17-40 us of K loop), the copy + its two barriers were ~3 us of each
  constexpr bool GRES = GDN && NPG == 4;
  const __amdgpu_buffer_rsrc_t gimage_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(GDN ? c.gdn_image : nullptr), 0, GDN ? GDN_IMAGE_BYTES : 0, 0x00020000);
  // y = convolution + bias as the bfloat16 tensor would hold it, packed (K step s of the contraction is xb[p][s] with the
  // sign bits cleared); the epilogue multiplies it with the norm's power as it packs the output — the 192 results of a
  // lane never exist at once (as a loop of their own they sat in registers beside y: 50 of them went to scratch, and
  // the reloads, each waited for, were 13 us of every item, tools/conv3_clock_probe.py)
  unsigned int xb[GDN ? MT : 1][GDN ? 2 * TILES : 1][4];      // (single words: four-register tuples of them made the allocator spill)
  auto gdn_stage = [&]() __attribute__((always_inline)) {
    constexpr int KT = TILES, KS = 2 * TILES;
    unsigned char* const gl = smem + d.oimage;
    const float* const bias_s = reinterpret_cast<const float*>(smem + d.obias);      // (zeros without a bias)
    constexpr int R0 = (GDN_PIECES + 1) / 2;
    u32x4 g1[GRES ? 1 : GDN_PIECES - R0];
    if constexpr (!GRES) {
      // the image -> LDS over the weight buffers, in two rounds of requests (registers); only the image's bytes are
      // written (the bias sits behind it)
      TFC_LDS_BARRIER();                  // every wave is through with the weight buffers
      {
        u32x4 g0[R0];
#pragma unroll
        for (int i = 0; i < R0; ++i) g0[i] = __builtin_amdgcn_raw_buffer_load_b128(gimage_rsrc, tid * 16u, i * TPIECE, 0);
#pragma unroll
        for (int i = 0; i < R0; ++i) *reinterpret_cast<u32x4*>(gl + i * TPIECE + tid * 16) = g0[i];
      }
#pragma unroll
      for (int i = R0; i < GDN_PIECES; ++i) g1[i - R0] = __builtin_amdgcn_raw_buffer_load_b128(gimage_rsrc, tid * 16u, i * TPIECE, 0);
    }
    // (under the second round of the image) y, packed; the accumulators are then free to take the norm
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int t0 = s >> 1, q0 = 2 * (s & 1);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_s + 32 * t0 + 8 * (q0 + half) + 4 * h);
        const int e = 4 * (q0 + half);
#pragma unroll
        for (int p = 0; p < MT; ++p) {
          xb[p][s][2 * half] = pack_bf16(acc[p][t0][e] + b4[0], acc[p][t0][e + 1] + b4[1]);
          xb[p][s][2 * half + 1] = pack_bf16(acc[p][t0][e + 2] + b4[2], acc[p][t0][e + 3] + b4[3]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);      // (16 channels at a time: registers)
    }
    if constexpr (!GRES) {
#pragma unroll
      for (int i = R0; i < GDN_PIECES; ++i)
        if (i * TPIECE + tid * 16 < GDN_IMAGE_BYTES) *reinterpret_cast<u32x4*>(gl + i * TPIECE + tid * 16) = g1[i - R0];
    }
    zero_acc();
    if constexpr (!GRES) TFC_LDS_BARRIER();
    TFC_CONV3_CLOCK(6);
    const bf16x8* const afr = reinterpret_cast<const bf16x8*>(gl) + lane;
    // gamma's fragments in the order they are used, (s, t) = (f / KT, f % KT), through a ring of four (three reads ahead:
    // a fragment serves two MFMAs, 64 cycles, an LDS read is ~150 away) — a whole K step of them ahead took 48 registers
    bf16x8 ring[4];
    auto frag_at = [&](int f) -> bf16x8 { return afr[((f % KT) * KS + f / KT) * 64]; };
#pragma unroll
    for (int f = 0; f < 3; ++f) ring[f] = frag_at(f);
    bf16x8 bfrag[MT];
#pragma unroll
    for (int f = 0; f < KS * KT; ++f) {
      const int s = f / KT, t = f % KT;
      if (f + 3 < KS * KT) ring[(f + 3) & 3] = frag_at(f + 3);
      if (t == 0) {
#pragma unroll
        for (int p = 0; p < MT; ++p)
          bfrag[p] = __builtin_bit_cast(bf16x8, u32x4{xb[p][s][0] & 0x7FFF7FFFu, xb[p][s][1] & 0x7FFF7FFFu,
                                                       xb[p][s][2] & 0x7FFF7FFFu, xb[p][s][3] & 0x7FFF7FFFu});
      }
#pragma unroll
      for (int p = 0; p < MT; ++p)
        acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[f & 3], bfrag[p], acc[p][t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    TFC_CONV3_CLOCK(7);
  };
  auto epilogue = [&](const Item& it, const int pb_last) __attribute__((always_inline)) {
    if constexpr (GDN) gdn_stage();
    // Output through LDS, a wave for itself.  The accumulators of a lane are 4 (+ 4 of its partner half) consecutive
    // channels of ONE pixel: stored straight from them, an instruction is 32 pixels x 32 bytes — 32 partial lines, ~50
    // cycles each in the CU's store path, 9-10 us per item (tools/conv3_clock_probe.py).  Instead one 128-byte line per
    // pixel at a time (bfloat16: two column tiles, float32: one) goes to the wave's 8 KB of the staging area as
    // [pixel][8 granules], granule g at g ^ (pixel / 2 & 7) (16 lanes of a ds_write_b128 / ds_read_b128: all banks
    // once), and leaves as 8 pixels x 128 bytes per instruction: whole lines.  The bias comes from LDS (parked there by
    // the prologue, zeros without one): a global load here would wait, in vmcnt order, for every store issued before
    // it.  Straight-line code: pixels outside the map get a buffer offset outside the image (the store is dropped).
    static_assert(TILES % 2 == 0, "two column tiles per output line");
    static_assert(!(GDN && OUTF32), "float32 output: no fused GDN");
    // (d.ostage < 0: no room of its own — the patch buffer of the LAST channel block instead: every read of it was
    // complete at the K loop's last barrier, the loop's last K step reads ahead into the other buffers only)
    // (d.ostage == -2, builds with the GDN image resident: the weight buffers — what the last K step reads ahead from
    // them is never used)
    unsigned char* const ost = smem + (d.ostage >= 0 ? d.ostage : d.ostage == -2 ? static_cast<int>(2 * PATCH_BYTES)
                                                                                 : pb_last * static_cast<int>(PATCH_BYTES)) + wid * (MT * 4096);
    // what is added to an accumulator: the bias; with GDN the norm's beta (behind gamma's fragments in the image)
    const float* const bias_s = reinterpret_cast<const float*>(smem + (GDN ? d.oimage + TILES * 2 * TILES * 1024 : d.obias));
    const int phy = it.group / c.su, phx = it.group % c.su;       // a group = one output phase, all its Cout channels
    constexpr int ROUNDS = OUTF32 ? TILES : TILES / 2;
    constexpr int ESZ = OUTF32 ? 4 : 2;
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<unsigned char*>(y) + it.n * c.OH * c.OW * c.Cout * ESZ, 0, c.OH * c.OW * c.Cout * ESZ, 0x00020000);
    auto wave_sync = [&]() __attribute__((always_inline)) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto slot = [&](int pix, int g) -> unsigned char* { return ost + pix * 128 + ((g ^ ((pix >> 1) & 7)) << 4); };
    // where this lane's 8 read-back granules go: granule j = pixel 8 j + lane / 8 = row p = j / 4 of the wave's two,
    // column 8 (j & 3) + lane / 8 — 16 bytes at 16 (lane & 7) of its line.  Per row a lane offset (outside the image
    // for a row outside the map), the column step and the line of the round as the scalar offset
    unsigned int yrow[MT];
    const int qxl = it.qx0 + (lane >> 3);
#pragma unroll
    for (int p = 0; p < MT; ++p) {
      const int qy = it.qy0 + MT * wid + p;
      yrow[p] = qy < c.OHq ? static_cast<unsigned int>(((qy * c.su + phy) * c.OW + qxl * c.su + phx) * c.Cout * ESZ + 16 * (lane & 7))
                           : 0x80000000u;
    }
    const int xroom = c.OWq - qxl;                       // column 8 k of the lane is inside the map iff 8 k < xroom
    const unsigned int xstep = static_cast<unsigned int>(8 * c.su * c.Cout * ESZ);
    auto rounds = [&](auto relu_tag, auto inv_tag) __attribute__((always_inline)) {
      constexpr bool RELU = decltype(relu_tag)::value, INV = decltype(inv_tag)::value;
      auto bias4 = [&](int ch) -> f32x4 { return *reinterpret_cast<const f32x4*>(bias_s + ch + 4 * h); };
      // output value of accumulator element 4 q + r of (p, t): + bias; with GDN y / norm (IGDN: y * norm), norm = the
      // accumulator + beta, y = the packed word of the same channel
      auto elem = [&](int p, int t, int q, int r, const f32x4& b4) -> float {
        float v = acc[p][t][4 * q + r] + b4[r];
        if constexpr (GDN) {
          const unsigned int word = xb[p][2 * t + (q >> 1)][2 * (q & 1) + (r >> 1)];
          const float yv = __uint_as_float((r & 1) ? (word & 0xFFFF0000u) : (word << 16));
          v = yv * (INV ? v : __builtin_amdgcn_rcpf(v));
        }
        if (RELU) v = fmaxf(v, 0.f);
        return v;
      };
#pragma unroll
      for (int rd = 0; rd < ROUNDS; ++rd) {
        if constexpr (OUTF32) {
          const int t = rd;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 b4 = bias4(32 * t + 8 * q);
#pragma unroll
            for (int p = 0; p < MT; ++p) {
              f32x4 v;
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = elem(p, t, q, r, b4);
              *reinterpret_cast<f32x4*>(slot(32 * p + l, 2 * q + h)) = v;
            }
            __builtin_amdgcn_sched_barrier(0);        // 8 channels at a time (registers)
          }
        } else {
#pragma unroll
          for (int t2 = 0; t2 < 2; ++t2) {
            const int t = 2 * rd + t2;
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {
              const f32x4 be = bias4(32 * t + 16 * qp), bo = bias4(32 * t + 16 * qp + 8);
#pragma unroll
              for (int p = 0; p < MT; ++p) {
                u32x4 o;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                  const f32x4& b4 = half ? bo : be;      // channels 32 t + 16 qp + 8 half + 4 h + {0 .. 3}
                  float v[4];
#pragma unroll
                  for (int r = 0; r < 4; ++r) v[r] = elem(p, t, 2 * qp + half, r, b4);
                  o[2 * half] = pack_bf16(v[0], v[1]);
                  o[2 * half + 1] = pack_bf16(v[2], v[3]);
                }
                // the halves trade their inner words: this lane then holds channels 32 t + 16 qp + 8 h + {0 .. 7}
                const auto s0 = __builtin_amdgcn_permlane32_swap(o.x, o.z, false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(o.y, o.w, false, false);
                *reinterpret_cast<u32x4*>(slot(32 * p + l, 4 * t2 + 2 * qp + h)) = u32x4{s0[0], s1[0], s0[1], s1[1]};
              }
              __builtin_amdgcn_sched_barrier(0);      // 16 channels at a time (registers)
            }
          }
        }
        wave_sync();
#pragma unroll
        for (int p = 0; p < MT; ++p) {          // a row's four granules at a time (registers)
          u32x4 v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const u32x4*>(slot(32 * p + 8 * k + (lane >> 3), lane & 7));
#pragma unroll
          for (int k = 0; k < 4; ++k) {
#if TFC_CONV3_EXP & 32
            if (v[k].x != 0x12345u) continue;     // (no stores)
#endif
            // (non-temporal — cache policy 2 — where the output cannot stay in the caches: the lines do not displace the
            // patches and weights other workgroups are about to read)
            if (c.nt_out) __builtin_amdgcn_raw_buffer_store_b128(v[k], yr, 8 * k < xroom ? yrow[p] : 0x80000000u, 128 * rd + k * xstep, 2);
            else __builtin_amdgcn_raw_buffer_store_b128(v[k], yr, 8 * k < xroom ? yrow[p] : 0x80000000u, 128 * rd + k * xstep, 0);
          }
        }
        wave_sync();
      }
    };
    using T = std::true_type;
    using F = std::false_type;
    if constexpr (GDN) {
      rounds(F{}, std::integral_constant<bool, GDNK == 2>{});       // (no other activation beside the GDN)
    } else {
      if (c.activation == 1) rounds(T{}, F{}); else rounds(F{}, F{});
    }
  };

  // Schedule of a chunk c (CH K steps, weights in LDS buffer c & 1; the slots of every kind of staging: at channel_block):
  //   the next chunks' weights   WDMA: chunk c + 1 requested into buffer (c + 1) & 1 in chunk c's first K step (5-K-step
  //                chunks) or chunk c + 2 into buffer c & 1 in its last (shorter chunks) — either way into a buffer whose
  //                last readers finished before a barrier, and waited for (vmcnt) in front of the barrier that publishes it.
  //                Through registers (TFC_CONV3_WDMA = 0): requested a chunk earlier, registers -> LDS in the first K step
  //   first chunk of a channel block: the next channel block's patch requested
  //   K step kk    reads the fragments of K step kk + 1 under its MFMAs
  //   end of kk = CH - 2   (last chunk of a channel block: the patch registers -> the other patch buffer;) wait for
  //                this wave's LDS traffic, barrier
  //   kk = CH - 1  the fragments it reads ahead are those of chunk c + 1's first K step: from the buffers published
  //                before the barrier, so no K step ever waits for a read it has just issued behind a barrier
  // (no __syncthreads: its fence would also wait for the global prefetches in flight).
  constexpr int NT = CH * NCH;            // taps of a group = K steps of a channel block
  // (the first requests go out before the rest of the bookkeeping: it runs under their latency)
  const Item cur = item_at(u);
  unsigned int poff[NPT];
  const __amdgpu_buffer_rsrc_t wr = weight_rsrc(cur);
  wfetch(wr, 0);
  patch_offsets(cur.qx0, cur.qy0, poff);
  const __amdgpu_buffer_rsrc_t xr = image_rsrc(cur.n);
  pfetch(xr, poff, 0);
  // the taps' patch offsets (wave-uniform, one SGPR each: the K steps below are unrolled over a whole channel block)
  unsigned int toff[NT];
  auto tap_table = [&](const Item& it) __attribute__((always_inline)) {
    int uy = it.uy0, ux = it.ux0;           // tap k = (uy0 + k / wx, ux0 + k % wx), walked
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      toff[k] = tap_offset(uy, ux);
      if (++ux == it.ux1) { ux = it.ux0; ++uy; }
    }
  };
  tap_table(cur);
  if (tid < TILES * 8)           // the bias, zeros without one (the epilogue's; with GDN: added before its contraction)
    *reinterpret_cast<f32x4*>(smem + d.obias + tid * 16) =
        bias ? *reinterpret_cast<const f32x4*>(bias + tid * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (GRES) {          // gamma's fragment image, for the whole item
    u32x4 gi[GDN_PIECES];
#pragma unroll
    for (int i = 0; i < GDN_PIECES; ++i) gi[i] = __builtin_amdgcn_raw_buffer_load_b128(gimage_rsrc, tid * 16u, i * TPIECE, 0);
#pragma unroll
    for (int i = 0; i < GDN_PIECES; ++i)
      if (i * TPIECE + tid * 16 < GDN_IMAGE_BYTES) *reinterpret_cast<u32x4*>(smem + d.oimage + i * TPIECE + tid * 16) = gi[i];
  }
  pstore(0);
  wstore(0);
  if constexpr (WDMA && WEARLY) {
    // (chunk 1: requested by chunk 0's first K step)
  } else if constexpr (WDMA) {   // chunk 1 -> the second buffer, on its way while chunk 0 is worked on
#pragma unroll
    for (int pc = 0; pc < STAGE; ++pc)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wr, (__attribute__((address_space(3))) void*)(wl + WBUF_BYTES + wave_u * 1024 + pc * TPIECE), 16,
          CHUNK_FRAGS * 16u + tid * 16u + pc * TPIECE, 0, 0, 0);
  } else {
    wfetch(wr, 1);
  }
  TFC_LDS_BARRIER();
  TFC_CONV3_CLOCK(1);

  bf16x8 af[2][TILES];
  u32x4 bq[2][MT];
#pragma unroll
  for (int t = 0; t < TILES; ++t) af[0][t] = (reinterpret_cast<const bf16x8*>(wl) + lane)[t * 64];
#pragma unroll
  for (int p = 0; p < MT; ++p) bq[0][p] = *reinterpret_cast<const u32x4*>(smem + lb[p] + toff[0]);
  int gchunk = 0;                         // chunks so far: weight buffer gchunk & 1
  int pcb = 0;                            // channel blocks so far: patch buffer pcb & 1

  // ONE CHANNEL BLOCK: NT K steps in NCH weight chunks, fully unrolled — one basic block, so that the staging of a
  // chunk boundary (registers -> LDS, the next requests) and of the patch sits between the MFMAs of the K steps
  // around it, and a tap is a compile-time index into the offset table.  Schedule of chunk c (weights in LDS buffer
  // c & 1):
  //   first K step   chunk c + 1 (requested during chunk c - 1) registers -> LDS buffer (c + 1) & 1, whose last readers
  //                  finished before the barrier of chunk c - 1; request chunk c + 2; first chunk of the block: request
  //                  the next channel block's patch (the next ITEM's first, behind an item's last)
  //   K step kk      reads the fragments of K step kk + 1 under its MFMAs
  //   end of kk = CH - 2   (last chunk: the patch registers -> the other patch buffer;) LDS barrier
  //   kk = CH - 1    the fragments it reads ahead are those of chunk c + 1's first K step, from the buffers published
  //                  before the barrier: no K step waits for a read it has just issued behind a barrier
  // Fragment register sets alternate per K step; a block of an odd number of K steps ends with a copy so that every
  // block starts from set 0.
#if TFC_CONV3_EXP & 64
  long long kwait[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  // Where the staging sits inside a chunk (round 6).  A K step is TILES * MT SLOTS — one MFMA each (32 cycles of the
  // matrix pipe), the order pinned slot by slot (sched_barrier) — and every staging instruction of the wave gets a slot of
  // its own: as bursts in front of a chunk's first MFMA (eight 13-cycle ds_write_b128 with a vmcnt wait each, then 8 + NPG
  // buffer loads; the compiler's schedule, sched_group_barrier masks or not) the matrix pipe stood still for them — one
  // wave per SIMD, nobody else to issue — and the builds without them (TFC_CONV3_EXP 2 / 4) were 12 % / 18 % faster.
  //   every K step     slots 0 .. MT - 1: the next K step's B fragments, MT .. MT + TILES - 1: its A fragments
  //   K step 0         slots 0 .. STAGE - 1: weight chunk c + 1, registers -> LDS
  //   K step 1         slots 0 .. STAGE - 1: weight chunk c + 2 requested
  //   K step PFK of a block's first chunk: the next channel block's patch requested (none behind the last block: a
  //                    descriptor of no records — no traffic, zeros — instead of a branch in the block)
  //   K step CH - 2 of its last chunk: the patch registers -> the other patch buffer; then the LDS barrier
  constexpr int SLOTS = TILES * MT;
  constexpr int PFK = NCH == 1 ? 0 : (CH > 2 ? 2 : CH - 1);           // (one chunk per block: as early as possible)
  constexpr int PF0 = NCH == 1 ? STAGE : 0;                           // its first slot
  constexpr int PS0 = (CH - 2 == 0 || CH - 2 == 1) ? STAGE : 0;       // the patch store's first slot (behind the weights' of that step)
  static_assert(CH >= 3, "K steps 0, 1 and CH - 2 of a chunk carry its staging");
  // (piece pc of a kind whose first slot is F sits in slot (F + pc) % SLOTS: the 128-channel builds have 8 slots for 10
  // patch pieces)
  auto channel_block = [&](const int cbi, const int chunk0, const int wpar, const int pb)
                           __attribute__((always_inline)) {
    const bool more = cbi + 1 < cb;
    const unsigned char* pbase = smem + pb * PATCH_BYTES;
    const unsigned char* pnext = smem + (pb ^ 1) * PATCH_BYTES;
    unsigned char* const pdstb = smem + (pb ^ 1) * PATCH_BYTES;
    const __amdgpu_buffer_rsrc_t xrn = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__bf16*>(x + cur.n * c.H * c.W * c.Cin), 0, more ? c.H * c.W * c.Cin * 2 : 0, 0x00020000);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int buf = wpar ^ (ch & 1);
      const bf16x8* abase = reinterpret_cast<const bf16x8*>(wl + buf * WBUF_BYTES) + lane;
      const bf16x8* anext = reinterpret_cast<const bf16x8*>(wl + (buf ^ 1) * WBUF_BYTES) + lane;
      u32x4* const wdst = reinterpret_cast<u32x4*>(wl + (buf ^ 1) * WBUF_BYTES) + tid;
      unsigned char* const wdma = wl + (WEARLY ? buf ^ 1 : buf) * WBUF_BYTES + wave_u * 1024;      // this wave's KB of a piece (+ lane * 16: the hardware)
      const unsigned int wv0 = static_cast<unsigned int>(chunk0 + ch + 2) * (CHUNK_FRAGS * 16u) + tid * 16u;   // (past the last chunk: outside the buffer)
#if TFC_CONV3_EXP & 64
      {   // (timing build: the wait the first store below begins with, by hand)
        const long long w0 = clock64();
        if (NCH > 1 && ch == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPT) : "memory");      // (behind it: the patch gather)
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        kwait[4] += clock64() - w0;
      }
#endif
#pragma unroll
      for (int kk = 0; kk < CH; ++kk) {
        const int k = ch * CH + kk;
        const int cur_set = k & 1, nxt_set = cur_set ^ 1;
        const bool last_kk = kk + 1 == CH, block_end = ch + 1 == NCH;
        // the next K step's tap (the item's last step reads ahead for nothing)
        const unsigned int tn = last_kk ? toff[!block_end && k + 1 < NT ? k + 1 : 0] : toff[k + 1 < NT ? k + 1 : 0];
        const unsigned char* const bsrc = last_kk && block_end ? pnext : pbase;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
          const int t = i / MT, p = i % MT;
          acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              af[cur_set][t], __builtin_bit_cast(bf16x8, bq[cur_set][p]), acc[p][t], 0, 0, 0);
#pragma unroll
          for (int f = 0; f < MT + TILES; ++f) {          // fragment f of the next K step: B first, in slot f % SLOTS
            if (f % SLOTS != i) continue;
            if (f < MT) bq[nxt_set][f] = *reinterpret_cast<const u32x4*>(bsrc + lb[f] + tn);
            else af[nxt_set][f - MT] = last_kk ? anext[(f - MT) * 64] : abase[((kk + 1) * TILES + (f - MT)) * 64];
          }
#if !(TFC_CONV3_EXP & 2)
          if constexpr (WDMA) {
            // (a request past the item's last chunk is outside the weights' buffer: no traffic, zeros written; the one the
            // last K step makes is waited for behind the loop.  Under a condition instead, the branch cost 4 % of the layer)
            if (kk == (WEARLY ? 0 : CH - 1)) {
#pragma unroll
              for (int pc = 0; pc < STAGE; ++pc)
                if (pc % SLOTS == i)
                  TFC_CONV3_ISSUE(0, __builtin_amdgcn_raw_ptr_buffer_load_lds(
                                         wr, (__attribute__((address_space(3))) void*)(wdma + pc * TPIECE), 16,
                                         wv0 - (WEARLY ? CHUNK_FRAGS * 16u : 0u) + pc * TPIECE, 0, 0, 0));
            }
          } else {
            if (kk == 0) {
#pragma unroll
              for (int pc = 0; pc < STAGE; ++pc)
                if (pc % SLOTS == i) TFC_CONV3_ISSUE(2, wdst[pc * NTHR] = stage[pc]);
            }
            if (kk == 1) {
#pragma unroll
              for (int pc = 0; pc < STAGE; ++pc)
                if (pc % SLOTS == i) TFC_CONV3_ISSUE(0, stage[pc] = __builtin_amdgcn_raw_buffer_load_b128(wr, wv0 + pc * TPIECE, 0, 0));
            }
          }
#endif
#if !(TFC_CONV3_EXP & 4)
          if (ch == 0 && kk == PFK) {
#pragma unroll
            for (int pc = 0; pc < NPT; ++pc)
              if ((PF0 + pc) % SLOTS == i)
                TFC_CONV3_ISSUE(1, pst[pc] = __builtin_amdgcn_raw_buffer_load_b128(xrn, poff[pc], (cbi + 1) * 32, 0));
          }
          // requested in the block's first chunk, stored in its last: the gather has the whole block to arrive
          if (block_end && kk == CH - 2) {
#pragma unroll
            for (int pc = 0; pc < NPT; ++pc)
              if ((PS0 + pc) % SLOTS == i)
                TFC_CONV3_ISSUE(3, *reinterpret_cast<u32x4*>(pdstb + pdst[pc]) = pst[pc]);
          }
#endif
#if TFC_CONV3_EXP & 64
          if (i == SLOTS - 1) TFC_CONV3_ISSUE(7, (void)0);        // (calibration: the pair of clock reads by itself)
#endif
          __builtin_amdgcn_sched_barrier(0);
        }
        if (kk == CH - 2) {
          if constexpr (WDMA) {       // this wave's pieces of the next chunk have landed (behind them in the queue: a patch gather
                                      // requested in this chunk)
            if (ch == 0 && PFK <= CH - 2 && (!WEARLY || PFK > 0)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPT) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
#if !(TFC_CONV3_EXP & 1)
#if TFC_CONV3_EXP & 64
          const long long b0 = clock64();
          TFC_LDS_BARRIER();
          kwait[5] += clock64() - b0;
#else
          TFC_LDS_BARRIER();
#endif
#endif
        }
      }
    }
    if constexpr (NT & 1) {
#pragma unroll
      for (int t = 0; t < TILES; ++t) af[0][t] = af[1][t];
#pragma unroll
      for (int p = 0; p < MT; ++p) bq[0][p] = bq[1][p];
    }
  };
#if TFC_CONV3_EXP & 64
  const long long k0 = clock64();
#endif
  for (int cbi = 0; cbi < cb; ++cbi) {
    channel_block(cbi, cbi * NCH, gchunk & 1, pcb & 1);
    gchunk += NCH;
    ++pcb;
  }
#if TFC_CONV3_EXP & 64
  kwait[6] = clock64() - k0;
  if (threadIdx.x == 0 && blockIdx.x < kConv3ClockWgs)
    for (int i = 0; i < 8; ++i) g_conv3_waits[blockIdx.x * 8 + i] = kwait[i];
#endif
  if constexpr (WDMA && !WEARLY) {
    // the last K step's request (zeros for a chunk past the item's last) has landed before the epilogue takes LDS over —
    // with gamma's image resident its staging area IS the weight buffers, and another wave's piece may lie in this wave's
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (GRES) TFC_LDS_BARRIER();
  }
  TFC_CONV3_CLOCK(2);
  epilogue(cur, (pcb - 1) & 1);
#if TFC_CONV3_EXP & 64
  TFC_CONV3_CLOCK(3);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TFC_CONV3_CLOCK(4);
#endif
}

// Host side of the third-generation kernel: 0 = launched, -1 = not this shape (the caller goes on with the second
// generation), > 0 = error.
// TFC_CONV_GEN: 2 the second generation everywhere; 3 (default) the third on the transposed 5x5 layers of wide maps;
// 4 the third wherever it is built.  Measured on C4 (profiles/r03_notes.md): a step's convolutions take 31.0 instead of
// 34.0 ms alone on the chip, and with 8 steps in flight the step 40.8 instead of 43.0 ms (before the coder's workgroups
// were packed four waves to a CU it was the other way round, 48.8 against 47.0: the third generation's workgroups hold
// 152 KB of LDS and found even fewer CUs free of coder waves).  Read per call: tests compare the generations in one
// process.
#if TFC_CONV3_EXP & 64
extern "C" int tfc_debug_conv3_clocks(unsigned long long* out, int wgs) {
  if (wgs > kConv3ClockWgs) wgs = kConv3ClockWgs;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv3_clocks), sizeof(unsigned long long) * 8 * wgs) != hipSuccess) return -1;
  return wgs;
}
extern "C" int tfc_debug_conv3_waits(unsigned long long* out, int wgs) {
  if (wgs > kConv3ClockWgs) wgs = kConv3ClockWgs;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv3_waits), sizeof(unsigned long long) * 8 * wgs) != hipSuccess) return -1;
  return wgs;
}
#endif

static int conv3_gen() { return env_int("TFC_CONV_GEN", 3); }

int run_conv3(const __bf16* x, const float* w, const float* bias, __bf16* y, ConvGeom c, PackGeom g,
              unsigned long long key, hipStream_t st) {
  if (conv3_gen() < 3 || c.small_cin || (c.out_f32 && c.gdn) || c.Cin % 16 || (c.sd != 1 && c.sd != 2)) return -1;
  if (c.Cout != 128 && c.Cout != 192) return -1;
  // Where it is used (measured, tools/conv3_check.py and profiles/r03_notes.md): the transposed 5x5 layers, where it is
  // 18-25 % ahead of the second generation.  On the stride-2 analysis layers it is level with it (TFC_CONV_GEN=4 runs
  // it there): their patch is 4x the pixels per block and its 32-byte gathers re-fetch every 128-byte line of the input
  // once per channel block.  The rule looks at the map only, never at the batch: an image's result must not depend on
  // the batch it is coded in.
  // (small stride-2 maps — bls2017's 64x64 -> 32x32 at 512 images: 1.37 -> 1.26 ms — do not have that problem)
  const bool small_down = !g.up && c.sd == 2 && c.OWq * c.OHq <= 4096;
  // Since its workgroups take their blocks in XCD order (xcd_order: neighbouring blocks' patches meet in one L2) it is
  // ahead on the wide stride-2 maps too: 6.87-6.98 -> 6.32-6.37 ms at 384x256, 1.73-1.76 -> 1.57-1.61 at 192x128 (same
  // box, alternating; TFC_CONV_DOWN3=0 keeps those on the second generation).
  static const bool down3 = env_switch("TFC_CONV_DOWN3") != 0;
  const bool wide_down = down3 && !g.up && c.sd == 2 && c.xcd;
  if (conv3_gen() < 4 && !(g.up && c.su == 2) && !small_down && !wide_down) return -1;
  {
    const int bxn = (c.OWq + 31) / 32, byn = (c.OHq + 7) / 8;
    if (static_cast<double>(c.OWq) * c.OHq < 0.85 * (bxn * 32.0 * byn * 8.0)) return -1;   // blocks mostly outside the map
    if (bxn * byn < 4 && conv3_gen() < 4) return -1;                                       // a block or two per image
  }
  c.tiles = c.Cout / 32;
  c.groups = c.su * c.su;                              // one output phase per group
  if (c.groups > kMaxGroups) return -1;
  c.compact = 1;
  c.cbmajor = 1;
  const int cb = c.Cin / 16;
  int most = 0;
  for (int grp = 0; grp < c.groups; ++grp) {
    int taps = c.Uy * c.Ux;
    c.ty0[grp] = 0; c.ty1[grp] = c.Uy; c.tx0[grp] = 0; c.tx1[grp] = c.Ux;
    if (g.up && !(taps = phase_taps(c, g, grp, grp))) return -1;
    most = std::max(most, taps);
  }
  c.ksteps = most * cb;
  Conv3Geom d{};
  d.lg = c.sd == 2 ? 1 : 0;
  d.BXn = (c.OWq + 31) / 32;
  d.BYn = (c.OHq + 7) / 8;
  const int PH = 7 * c.sd + c.Uy;
  d.PW = 31 * c.sd + c.Ux;
  d.PWh = (d.PW + c.sd - 1) / c.sd;
  d.granules = PH * c.sd * 2 * d.PWh;
  d.pixels = PH * d.PW;
  fast_div_setup(d.BXn, &d.bx_mul, &d.bx_sh);
  fast_div_setup(d.BYn, &d.by_mul, &d.by_sh);
  fast_div_setup(d.PW, &d.pw_mul, &d.pw_sh);
  const int npg = 2 * ((d.pixels + 255) / 256);        // 16-byte pieces per thread: two per patch pixel
  const int npgt = npg <= 4 ? 4 : 10;                  // the built loader widths
  const size_t patch_bytes = static_cast<size_t>(npgt) * 4096 + (npgt > 4 ? 2048 : 0);
  if (npg > npgt || static_cast<size_t>(d.granules) * 16 + 16 * d.PWh + 16 > patch_bytes) return -1;
  // a launch per tap count: the kernel is built for 25 taps (5 chunks of 5 K steps; the big patch loader), and 9
  // (3 x 3), 6 (2 x 3), 4 (1 x 4) taps with the small one
  int nts[kMaxGroups];
  for (int grp = 0; grp < c.groups; ++grp) {
    nts[grp] = (c.ty1[grp] - c.ty0[grp]) * (c.tx1[grp] - c.tx0[grp]);
    const bool built = (nts[grp] == 25 && npgt == 10) || ((nts[grp] == 9 || nts[grp] == 6 || nts[grp] == 4) && npgt == 4);
    if (!built) return -1;
    if (cb * (nts[grp] == 25 ? 5 : nts[grp] == 9 ? 3 : nts[grp] == 6 ? 2 : 1) < 2) return -1;   // (weights are requested two chunks ahead)
  }
  DevBuf packed_local;
  DevView packed;
  const long long frags = static_cast<long long>(c.groups) * c.ksteps * c.tiles * 64;
  {
    const int rc = packed_weights(key, 1, {g.kh, g.kw, g.Cin_real, g.Cout, g.su, g.up, g.Uy, g.Ux, g.dmax_y, g.dmax_x, c.groups, c.ksteps,
                                      c.tiles, c.compact * 4 + c.cbmajor * 2 + c.small_cin, c.kw4},
                                  static_cast<size_t>(frags) * 16 + 64, st, packed_local, &packed.p, [&](void* dst) {
      launch_conv_pack(true, w, g, c, frags, dst, st);
      return 0;
    });
    if (rc) return rc;
  }
  KernelTimer timer("conv2d", st);
  const int tap_counts[4] = {25, 9, 6, 4};
  for (int ntv : tap_counts) {
    d.gcount = 0;
    for (int grp = 0; grp < c.groups; ++grp)
      if (nts[grp] == ntv) d.glist[d.gcount++] = grp;
    if (!d.gcount) continue;
    fast_div_setup(d.gcount, &d.gc_mul, &d.gc_sh);
    const int chv = ntv == 25 ? 5 : ntv == 4 ? 4 : 3;
    // LDS: two patch buffers | two weight chunks | with GDN as the activation gamma's fragment image + beta — over the
    // weight buffers (copied in by the GDN stage) in the big-patch builds, behind them for the whole item in the
    // small-patch ones | the bias | the epilogue's staging area (4 waves x 8 KB) where there is room; else it takes the
    // weight buffers (image resident: nothing of them is needed after the K loop) or the patch buffer the last channel
    // block has left (the kernel's comments)
    const size_t wbufs = 2 * static_cast<size_t>((chv * c.tiles * 64 + 255) / 256) * 4096;
    const size_t image_bytes = static_cast<size_t>(c.tiles) * 2 * c.tiles * 64 * 16 + static_cast<size_t>(c.tiles) * 32 * 4;
    const bool resident = c.gdn && npgt == 4;
    size_t lds_all = 2 * patch_bytes;
    d.oimage = static_cast<int>(lds_all);
    if (resident) {
      lds_all += wbufs;
      d.oimage = static_cast<int>(lds_all);
      lds_all += (image_bytes + 1023) / 1024 * 1024;
    } else {
      lds_all += std::max(wbufs, c.gdn ? image_bytes : size_t{0});
    }
    d.obias = static_cast<int>(lds_all);
    lds_all += 1024;
    if (lds_all + 32768 <= kLdsBytesPerCu) {
      d.ostage = static_cast<int>(lds_all);
      lds_all += 32768;
    } else if (resident && wbufs >= 32768) {
      d.ostage = -2;
    } else if (patch_bytes >= 32768) {
      d.ostage = -1;
    } else {
      return -1;
    }
    if (lds_all > kLdsBytesPerCu) return -1;
    // One workgroup per block and group.  (A grid of one workgroup per CU, each taking every W-th block, is the same
    // speed alone on the chip — round 6, with the cheaper epilogue: 2 % / 6 % ahead on the stride-2 / transposed layer —
    // but keeps the kernels of other steps in flight out of its CUs: C4 51.6 instead of 47.6 ms per step,
    // profiles/r03_notes.md.)
    static const int nt_env = env_switch("TFC_CONV_NT");
    c.nt_out = beyond_cache(c.N * c.OH * c.OW * c.Cout * (c.out_f32 ? 4 : 2), nt_env);
    const long long nblk = c.N * d.BXn * d.BYn * d.gcount;
    if (nblk > kMaxGridX) return fail("tfc_conv2d: problem too large for one launch");
    const dim3 grid(static_cast<unsigned>(nblk));
#define TFC_CONV3_LAUNCH_G(NT, CHV, NCHV, NPGV, G, F32)                                                    \
    do {                                                                                                   \
      if (int rc = launch(&conv3_bf16_kernel<NT, CHV, NCHV, NPGV, G, F32>, grid, dim3(256), lds_all, st, x, packed.p, bias, y, c, d)) \
        return rc;                                                                                         \
    } while (0)
#define TFC_CONV3_LAUNCH(NT, CHV, NCHV, NPGV)                                                              \
    do {                                                                                                   \
      if (c.out_f32) TFC_CONV3_LAUNCH_G(NT, CHV, NCHV, NPGV, 0, true);                                     \
      else if (c.gdn == 2) TFC_CONV3_LAUNCH_G(NT, CHV, NCHV, NPGV, 2, false);                              \
      else if (c.gdn) TFC_CONV3_LAUNCH_G(NT, CHV, NCHV, NPGV, 1, false);                                   \
      else TFC_CONV3_LAUNCH_G(NT, CHV, NCHV, NPGV, 0, false);                                              \
    } while (0)
#define TFC_CONV3_TAPS(NT)                                                   \
    do {                                                                     \
      if (ntv == 25) TFC_CONV3_LAUNCH(NT, 5, 5, 10);                         \
      else if (ntv == 9) TFC_CONV3_LAUNCH(NT, 3, 3, 4);                      \
      else if (ntv == 6) TFC_CONV3_LAUNCH(NT, 3, 2, 4);                      \
      else TFC_CONV3_LAUNCH(NT, 4, 1, 4);                                    \
    } while (0)
    if (c.tiles == 6) TFC_CONV3_TAPS(6); else TFC_CONV3_TAPS(4);
#undef TFC_CONV3_TAPS
#undef TFC_CONV3_LAUNCH
#undef TFC_CONV3_LAUNCH_G
  }
  return 0;
}

}  // namespace tfc
