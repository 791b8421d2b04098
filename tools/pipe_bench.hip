// Standalone harness for the deep-pipelined GEMM work (round 2):
//   --probe   dump ds_read_b64_tr_b16 per-lane gather semantics (the HW
//             transpose read planned for the TN-operand pipeline)
//   --epi     scalar vs 16-byte-store epilogue timing at the ResNet101
//             bs64 shapes (mix_gemm.h vec_epilogue_band)
//   default   numerics check (CPU f64 ref at small sizes) + TF sweep of
//             gemm256 (round-1) vs pipe256 swizzle/barrier variants at
//             4096³/8192³ bf16 on uniform random [-1,1) operands
//             (guide §5.4 rule 25: quote the random-data number).
//
// Build: hipcc --offload-arch=gfx950 -O3 tools/pipe_bench.hip -o tools/pipe_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../mpi_operator_amd/ops/csrc/mfma_tile.h"
#include "../mpi_operator_amd/ops/csrc/mix_gemm.h"

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e = (x);                                                       \
    if (e != hipSuccess) {                                                    \
      fprintf(stderr, "HIP error %s @%d\n", hipGetErrorString(e), __LINE__);  \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

// ---- tr_b16 probe ----------------------------------------------------
typedef __attribute__((ext_vector_type(2))) unsigned int uint2v;

// LDS halfwords filled with their own index; lane t reads at byte addr
// t*8 (pattern A) or custom patterns; output shows which 4 halfword
// indices land in each lane.
__global__ void tr_probe_k(unsigned int *out, int pattern) {
  __shared__ unsigned short l[2048];
  int t = threadIdx.x;
  // volatile: the array address only reaches the asm as an integer, so
  // without this the compiler proves the fill dead and drops the LDS
  // allocation entirely (observed: group_segment_fixed_size 0)
  volatile unsigned short *vl = l;
  for (int i = t; i < 2048; i += 64) vl[i] = i;
  __syncthreads();
  unsigned int off;
  if (pattern == 0) off = t * 8;                   // lane-linear 8 B
  else if (pattern == 1) off = (t & 15) * 8;       // group-constant rows
  else off = ((t & 15) * 4 + (t >> 4) * 64) * 2;   // guide layout guess
  // address = LDS byte offset of l + per-lane offset (AS3 cast)
  unsigned int addr =
      (unsigned int)(unsigned long)(__attribute__((address_space(3)))
                                    unsigned short *)l + off;
  uint2v v;
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)"
               : "=v"(v) : "v"(addr) : "memory");
  out[t * 2] = v.x;
  out[t * 2 + 1] = v.y;
}

static void run_probe() {
  unsigned int *d;
  CHECK(hipMalloc(&d, 64 * 2 * sizeof(unsigned int)));
  std::vector<unsigned int> h(128);
  for (int pat = 0; pat < 3; ++pat) {
    tr_probe_k<<<1, 64>>>(d, pat);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), d, 128 * 4, hipMemcpyDeviceToHost));
    printf("tr_b16 pattern %d (halfword indices per lane):\n", pat);
    for (int l = 0; l < 64; ++l) {
      unsigned short a = h[l * 2] & 0xffff, b = h[l * 2] >> 16;
      unsigned short c = h[l * 2 + 1] & 0xffff, e = h[l * 2 + 1] >> 16;
      printf("  lane %2d: %4d %4d %4d %4d\n", l, a, b, c, e);
    }
  }
  hipFree(d);
}

// ---- GEMM numerics + perf --------------------------------------------
static uint16_t f2bf_h(float f) {
  union { float f; uint32_t i; } v;
  v.f = f;
  uint32_t lsb = (v.i >> 16) & 1u;
  v.i += 0x7fffu + lsb;
  return uint16_t(v.i >> 16);
}
static float bf2f_h(uint16_t u) {
  union { uint32_t i; float f; } v;
  v.i = uint32_t(u) << 16;
  return v.f;
}

enum Variant {
  V_GEMM256, V_PIPE_S0, V_PIPE_S1, V_PIPE_S2, V_PIPE_S1_1B,
  V_PIPE_SPRIO, V_PIPE_1B_SPRIO, N_VAR
};
static const char *vname[] = {"gemm256(r1)", "pipe swz0", "pipe swz1",
                              "pipe swz2", "pipe swz1 1bar",
                              "pipe sprio", "pipe 1bar+sprio"};

static hipError_t launch_variant(int v, const uint16_t *a, const uint16_t *b,
                                 float *c, int M, int N, int K) {
  GemmLoader la{a, M, (long)K, K};
  GemmLoader lb{b, N, (long)K, K};
  int tiles_n = N / 256;
  int nwg = (M / 256) * tiles_n;
  int cpx = (nwg % 8 == 0 && nwg >= 32) ? nwg / 8 : 0;
  switch (v) {
  case V_GEMM256:
    return launch_nt256(la, lb, c, M, N, K, N, true, 0);
  case V_PIPE_S0:
    pipe256_gemm_k<true, false, 0><<<nwg, 512>>>(a, (long)K, b, (long)K, c, M,
                                                 N, K, N, tiles_n, cpx, 0);
    break;
  case V_PIPE_S1:
    pipe256_gemm_k<true, false, 1><<<nwg, 512>>>(a, (long)K, b, (long)K, c, M,
                                                 N, K, N, tiles_n, cpx, 0);
    break;
  case V_PIPE_S2:
    pipe256_gemm_k<true, false, 2><<<nwg, 512>>>(a, (long)K, b, (long)K, c, M,
                                                 N, K, N, tiles_n, cpx, 0);
    break;
  case V_PIPE_S1_1B:
    pipe256_gemm_k<true, false, 1, 1><<<nwg, 512>>>(a, (long)K, b, (long)K, c,
                                                    M, N, K, N, tiles_n, cpx, 0);
    break;
  case V_PIPE_SPRIO:
    pipe256_gemm_k<true, false, 1, 2, 1><<<nwg, 512>>>(
        a, (long)K, b, (long)K, c, M, N, K, N, tiles_n, cpx, 0);
    break;
  case V_PIPE_1B_SPRIO:
    pipe256_gemm_k<true, false, 1, 1, 1><<<nwg, 512>>>(
        a, (long)K, b, (long)K, c, M, N, K, N, tiles_n, cpx, 0);
    break;
  }
  return hipGetLastError();
}

static int check_small(int M, int N, int K) {
  std::vector<uint16_t> ha(M * (long)K), hb(N * (long)K);
  srand(7);
  for (auto &x : ha) x = f2bf_h((rand() / (float)RAND_MAX) * 2 - 1);
  for (auto &x : hb) x = f2bf_h((rand() / (float)RAND_MAX) * 2 - 1);
  uint16_t *da, *db;
  float *dc;
  CHECK(hipMalloc(&da, ha.size() * 2));
  CHECK(hipMalloc(&db, hb.size() * 2));
  CHECK(hipMalloc(&dc, (long)M * N * 4));
  CHECK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(db, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  std::vector<float> ref((long)M * N);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      double s = 0;
      for (int k = 0; k < K; ++k)
        s += (double)bf2f_h(ha[(long)i * K + k]) * bf2f_h(hb[(long)j * K + k]);
      ref[(long)i * N + j] = (float)s;
    }
  std::vector<float> out((long)M * N);
  int fails = 0;
  for (int v = 1; v < N_VAR; ++v) {
    CHECK(hipMemset(dc, 0, (long)M * N * 4));
    CHECK(launch_variant(v, da, db, dc, M, N, K));
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), dc, (long)M * N * 4, hipMemcpyDeviceToHost));
    float maxerr = 0, scale = 0;
    for (long i = 0; i < (long)M * N; ++i) {
      float e = fabsf(out[i] - ref[i]);
      if (e > maxerr) maxerr = e;
      if (fabsf(ref[i]) > scale) scale = fabsf(ref[i]);
    }
    bool ok = maxerr < 0.01f * scale + 0.05f;
    printf("numerics %dx%dx%d %-14s maxerr %.4g scale %.3g %s\n", M, N, K,
           vname[v], maxerr, scale, ok ? "OK" : "FAIL");
    if (!ok) ++fails;
  }
  hipFree(da); hipFree(db); hipFree(dc);
  return fails;
}

static void bench(int M, int N, int K, int iters) {
  uint16_t *da, *db;
  float *dc;
  CHECK(hipMalloc(&da, (long)M * K * 2));
  CHECK(hipMalloc(&db, (long)N * K * 2));
  CHECK(hipMalloc(&dc, (long)M * N * 4));
  { // random fill on device (cheap LCG kernel via memset trick is wrong —
    // do host fill once; 4k² bf16 = 32 MB, fine)
    std::vector<uint16_t> h((long)M * K);
    srand(11);
    for (auto &x : h) x = f2bf_h((rand() / (float)RAND_MAX) * 2 - 1);
    CHECK(hipMemcpy(da, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    h.resize((long)N * K);
    for (auto &x : h) x = f2bf_h((rand() / (float)RAND_MAX) * 2 - 1);
    CHECK(hipMemcpy(db, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  }
  double flops = 2.0 * M * N * K;
  for (int v = 0; v < N_VAR; ++v) {
    CHECK(launch_variant(v, da, db, dc, M, N, K)); // warmup
    CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    for (int i = 0; i < iters; ++i)
      launch_variant(v, da, db, dc, M, N, K);
    hipEventRecord(e1);
    CHECK(hipEventSynchronize(e1));
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    printf("perf %5dx%5dx%5d %-14s %8.1f TF (%.3f ms)\n", M, N, K, vname[v],
           flops * iters / (ms * 1e-3) / 1e12, ms / iters);
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  hipFree(da); hipFree(db); hipFree(dc);
}

// ---- TN-pipeline (pipe_mix) numerics + perf ---------------------------
// variants: 0 = mix_gemm (round-1 register-staged), 1 = pipe_mix
static hipError_t launch_tn(int v, int kind, const uint16_t *a,
                            const uint16_t *b, float *c, int M, int N, int K,
                            int splits) {
  // kind 0: TN×TN (wgrad/linear-dw shape: A k-strided [K][M], B [K][N])
  // kind 1: NT×TN (dx shape: A [M][K], B [K][N])
  if (kind == 0) {
    if (v == 0) {
      TnRowMajor la{a, (long)M, K, M};
      TnRowMajor lb{b, (long)N, K, N};
      return launch_mix_gemm(TnStage<TnRowMajor>{la}, TnStage<TnRowMajor>{lb},
                             c, M, N, K, N, true, 0, splits);
    }
    TnPipe<PlainTnSrc> sa{{a, (long)M, K, M}};
    TnPipe<PlainTnSrc> sb{{b, (long)N, K, N}};
    return launch_pipe_mix_wr(sa, sb, c, M, N, K, LinearWriter{(long)N}, N,
                              true, 0, splits);
  }
  if (v == 0) {
    GemmLoader la{a, M, (long)K, K};
    TnRowMajor lb{b, (long)N, K, N};
    return launch_mix_gemm(NtStage<GemmLoader>{la}, TnStage<TnRowMajor>{lb},
                           c, M, N, K, N, true, 0, splits);
  }
  NtPipe<PlainNtSrc> sa{{a, (long)K, M, K}};
  TnPipe<PlainTnSrc> sb{{b, (long)N, K, N}};
  return launch_pipe_mix_wr(sa, sb, c, M, N, K, LinearWriter{(long)N}, N,
                            true, 0, splits);
}

static int check_tn(int kind, int M, int N, int K, int splits) {
  std::vector<uint16_t> ha, hb;
  srand(13 + kind);
  // A: kind 0 → [K][M]; kind 1 → [M][K].  B: [K][N]
  ha.resize((long)M * K);
  hb.resize((long)N * K);
  for (auto &x : ha) x = f2bf_h((rand() / (float)RAND_MAX) * 2 - 1);
  for (auto &x : hb) x = f2bf_h((rand() / (float)RAND_MAX) * 2 - 1);
  uint16_t *da, *db;
  float *dc, *dpart = nullptr;
  CHECK(hipMalloc(&da, ha.size() * 2));
  CHECK(hipMalloc(&db, hb.size() * 2));
  CHECK(hipMalloc(&dc, (long)M * N * 4));
  CHECK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(db, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  std::vector<float> ref((long)M * N, 0.f);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < M; ++i) {
      float av = bf2f_h(kind == 0 ? ha[(long)k * M + i] : ha[(long)i * K + k]);
      if (av == 0.f) continue;
      for (int j = 0; j < N; ++j)
        ref[(long)i * N + j] += av * bf2f_h(hb[(long)k * N + j]);
    }
  int fails = 0;
  std::vector<float> out((long)M * N);
  for (int v = 0; v < 2; ++v) {
    CHECK(hipMemset(dc, 0, (long)M * N * 4));
    if (splits > 1) { // host-side slab reduce (the tool has no conv.hip TU)
      CHECK(hipMalloc(&dpart, (long)splits * M * N * 4));
      CHECK(launch_tn(v, kind, da, db, dpart, M, N, K, splits));
      CHECK(hipDeviceSynchronize());
      std::vector<float> slabs((long)splits * M * N);
      CHECK(hipMemcpy(slabs.data(), dpart, slabs.size() * 4,
                      hipMemcpyDeviceToHost));
      for (long i = 0; i < (long)M * N; ++i) {
        float sum = 0;
        for (int sp = 0; sp < splits; ++sp) sum += slabs[(long)sp * M * N + i];
        out[i] = sum;
      }
      hipFree(dpart);
    } else {
      CHECK(launch_tn(v, kind, da, db, dc, M, N, K, 1));
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(out.data(), dc, (long)M * N * 4, hipMemcpyDeviceToHost));
    }
    float maxerr = 0, scale = 0;
    for (long i = 0; i < (long)M * N; ++i) {
      float e = fabsf(out[i] - ref[i]);
      if (e > maxerr) maxerr = e;
      if (fabsf(ref[i]) > scale) scale = fabsf(ref[i]);
    }
    bool ok = maxerr < 0.01f * scale + 0.05f;
    printf("tn-numerics kind%d %dx%dx%d sk%d %-8s maxerr %.4g %s\n", kind, M,
           N, K, splits, v ? "pipe_mix" : "mix", maxerr, ok ? "OK" : "FAIL");
    if (!ok) {
      ++fails;
      // per-128x128-tile / per-wave-quadrant breakdown localizes the bug:
      // tile = which block; 64x64 quadrant within tile = which wave
      for (int tr_ = 0; tr_ < (M + 127) / 128; ++tr_)
        for (int tc = 0; tc < (N + 127) / 128; ++tc) {
          float te = 0;
          int bi = -1, bj = -1;
          for (int i = tr_ * 128; i < M && i < tr_ * 128 + 128; ++i)
            for (int j = tc * 128; j < N && j < tc * 128 + 128; ++j) {
              float e = fabsf(out[(long)i * N + j] - ref[(long)i * N + j]);
              if (e > te) { te = e; bi = i; bj = j; }
            }
          if (te > 0.05f)
            printf("  tile(%d,%d) maxerr %.3g at (%d,%d) got %.4f want %.4f "
                   "[quad %d,%d]\n", tr_, tc, te, bi, bj,
                   bi >= 0 ? out[(long)bi * N + bj] : 0.f,
                   bi >= 0 ? ref[(long)bi * N + bj] : 0.f,
                   bi >= 0 ? (bi % 128) / 64 : -1, bj >= 0 ? (bj % 128) / 64 : -1);
        }
    }
  }
  hipFree(da); hipFree(db); hipFree(dc);
  return fails;
}

static void bench_tn(int kind, int M, int N, int K, int splits, int iters) {
  uint16_t *da, *db;
  float *dc;
  CHECK(hipMalloc(&da, (long)M * K * 2));
  CHECK(hipMalloc(&db, (long)N * K * 2));
  CHECK(hipMalloc(&dc, (long)(splits > 1 ? splits : 1) * M * N * 4));
  CHECK(hipMemset(da, 0x3c, (long)M * K * 2)); // ~bf16 1.06: nonzero data
  CHECK(hipMemset(db, 0x3c, (long)N * K * 2));
  double flops = 2.0 * M * N * K;
  for (int v = 0; v < 2; ++v) {
    CHECK(launch_tn(v, kind, da, db, dc, M, N, K, splits));
    CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    for (int i = 0; i < iters; ++i)
      launch_tn(v, kind, da, db, dc, M, N, K, splits);
    hipEventRecord(e1);
    CHECK(hipEventSynchronize(e1));
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    printf("tn-perf kind%d %6dx%6dx%7d sk%-2d %-8s %8.1f TF (%.3f ms)\n",
           kind, M, N, K, splits, v ? "pipe_mix" : "mix",
           flops * iters / (ms * 1e-3) / 1e12, ms / iters);
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  hipFree(da); hipFree(db); hipFree(dc);
}

// ---- TN stage/read isolation debug ------------------------------------
// Stage ONE k-half of a [K][cols] matrix filled with value k*1000+col via
// TnPipe::stage, then (a) dump raw LDS halfwords, (b) dump what
// TnPipe::read delivers per lane — separates a staging-layout bug from a
// tr-read bug without the pipeline.
__global__ void tn_debug_k(const uint16_t *src, long ld, int kdim, int cols,
                           uint16_t *raw, uint16_t *frag,
                           const uint16_t *zeros, int base) {
  __shared__ __align__(128) ushort8 lds[PM_HSZ];
  TnPipe<PlainTnSrc> s{{src, ld, kdim, cols}};
  int tid = threadIdx.x;
  s.init(tid, base);
  s.stage(tid, 0, lds, zeros);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // (a) raw image: 512 slots x 8 halfwords (each thread dumps 2 slots)
  {
    ushort8 v = lds[tid];
    for (int j = 0; j < 8; ++j) raw[tid * 8 + j] = v[j];
    v = lds[256 + tid];
    for (int j = 0; j < 8; ++j) raw[(256 + tid) * 8 + j] = v[j];
  }
  __syncthreads();
  // (b) frag reads: waves pretend to be (wr=0..), frag0 0/32/64/96, ks 0/1
  int lane = tid & 63, wave = tid >> 6;
  int frag0 = wave * 32; // 4 waves cover frag0 = 0,32,64,96
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 v = s.read(lds, lane, frag0, ks);
    union { bf16x8 b; uint16_t u[8]; } u;
    u.b = v;
    for (int j = 0; j < 8; ++j)
      frag[((wave * 2 + ks) * 64 + lane) * 8 + j] = u.u[j];
  }
}

static void run_tn_debug() {
  int K = 32, cols = 128;
  std::vector<uint16_t> h(K * cols);
  for (int k = 0; k < K; ++k)
    for (int c = 0; c < cols; ++c) h[k * cols + c] = (uint16_t)(k * 200 + c);
  uint16_t *dsrc, *draw, *dfrag, *dz;
  CHECK(hipMalloc(&dsrc, h.size() * 2));
  CHECK(hipMalloc(&draw, 4096 * 2));
  CHECK(hipMalloc(&dfrag, 8 * 64 * 8 * 2));
  CHECK(hipMalloc(&dz, 256));
  CHECK(hipMemset(dz, 0, 256));
  CHECK(hipMemcpy(dsrc, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  tn_debug_k<<<1, PM_THREADS>>>(dsrc, cols, K, cols, draw, dfrag, dz, 0);
  CHECK(hipDeviceSynchronize());
  std::vector<uint16_t> raw(4096), frag(8 * 64 * 8);
  CHECK(hipMemcpy(raw.data(), draw, raw.size() * 2, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(frag.data(), dfrag, frag.size() * 2, hipMemcpyDeviceToHost));
  // expected raw: slot idx -> subtile st=idx>>3 (kq=st>>3,cq=st&7),
  // kl=(idx&7)>>1, ch=idx&1: halfword j = (kq*4+kl)*200 + cq*16+ch*8+j
  int bad = 0;
  for (int idx = 0; idx < 512 && bad < 10; ++idx) {
    int st = idx >> 3, kq = st >> 3, cq = st & 7;
    int kl = (idx & 7) >> 1, ch = idx & 1;
    for (int j = 0; j < 8; ++j) {
      uint16_t want = (uint16_t)((kq * 4 + kl) * 200 + cq * 16 + ch * 8 + j);
      if (raw[idx * 8 + j] != want) {
        printf("RAW MISMATCH idx %d j %d: got %d want %d\n", idx, j,
               raw[idx * 8 + j], want);
        ++bad;
        break;
      }
    }
  }
  if (!bad) printf("raw LDS image: OK (all 512 slots)\n");
  // expected frag: lane l of frag0 f, ks: row f+(l&31), k = ks*16+(l>>5)*8+j
  bad = 0;
  for (int w = 0; w < 4 && bad < 12; ++w)
    for (int ks = 0; ks < 2; ++ks)
      for (int l = 0; l < 64; ++l) {
        int f0 = w * 32;
        int col = f0 + (l & 31);
        for (int j = 0; j < 8; ++j) {
          int k = ks * 16 + (l >> 5) * 8 + j;
          uint16_t want = (uint16_t)(k * 200 + col);
          uint16_t got = frag[((w * 2 + ks) * 64 + l) * 8 + j];
          if (got != want) {
            printf("FRAG MISMATCH w%d ks%d lane%d j%d: got %d want %d\n", w,
                   ks, l, j, got, want);
            ++bad;
            break;
          }
        }
      }
  if (!bad) printf("tr_b16 frag reads: OK (4 frag0 x 2 ks x 64 lanes)\n");
  hipFree(dsrc); hipFree(draw); hipFree(dfrag); hipFree(dz);
}

// ---- mix-vs-pipe device cross-check at exact model shapes -------------
// mix_gemm is the round-1-trusted oracle; both paths accumulate fp32 in
// identical k order, so outputs should agree to ~bf16 rounding exactly.
// kind: 0 TN×TN, 1 NT×TN, 2 NT×TN with LinearAccWriter (dgrad-acc)
static int xcheck(int kind, long M, int N, int K, int splits) {
  uint16_t *da, *db, *dacc0 = nullptr;
  float *dc0, *dc1;
  CHECK(hipMalloc(&da, (long)M * K * 2));
  CHECK(hipMalloc(&db, (long)N * K * 2));
  long csz = (long)(splits > 1 ? splits : 1) * M * N;
  CHECK(hipMalloc(&dc0, csz * 4));
  CHECK(hipMalloc(&dc1, csz * 4));
  // deterministic pseudo-random bf16 fill on host (values in ±2)
  {
    std::vector<uint16_t> h((long)M * K);
    unsigned x = 0x1234567u;
    for (auto &v : h) {
      x = x * 1664525u + 1013904223u;
      v = f2bf_h(((x >> 8) & 0xffff) / 32768.0f - 1.0f);
    }
    CHECK(hipMemcpy(da, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    h.resize((long)N * K);
    for (auto &v : h) {
      x = x * 1664525u + 1013904223u;
      v = f2bf_h(((x >> 8) & 0xffff) / 32768.0f - 1.0f);
    }
    CHECK(hipMemcpy(db, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  }
  auto run_path = [&](int v, float *dc) -> hipError_t {
    if (kind == 2) { // acc: bf16 += ; dc reused as bf16 buffer
      CHECK(hipMemset(dc, 0x11, M * N * 2)); // same nonzero init both paths
      if (v == 0) {
        GemmLoader la{da, (int)M, (long)K, K};
        TnRowMajor lb{db, (long)N, K, N};
        return launch_mix_gemm_wr(NtStage<GemmLoader>{la},
                                  TnStage<TnRowMajor>{lb}, dc, (int)M, N, K,
                                  LinearAccWriter{(long)N}, N, false, 0);
      }
      NtPipe<PlainNtSrc> sa{{da, (long)K, (int)M, K}};
      TnPipe<PlainTnSrc> sb{{db, (long)N, K, N}};
      return launch_pipe_mix_wr(sa, sb, dc, (int)M, N, K,
                                LinearAccWriter{(long)N}, N, false, 0);
    }
    return launch_tn(v, kind, da, db, dc, (int)M, N, K, splits);
  };
  int bad = 0;
  CHECK(run_path(0, dc0));
  CHECK(hipDeviceSynchronize());
  CHECK(run_path(1, dc1));
  CHECK(hipDeviceSynchronize());
  long n_out = kind == 2 ? (M * N + 1) / 2 : csz; // acc compares bf16 pairs
  std::vector<float> h0(n_out), h1(n_out);
  CHECK(hipMemcpy(h0.data(), dc0, n_out * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(h1.data(), dc1, n_out * 4, hipMemcpyDeviceToHost));
  long diffs = 0;
  float maxd = 0;
  long first = -1;
  for (long i = 0; i < n_out; ++i) {
    float d = fabsf(h0[i] - h1[i]);
    if (kind == 2) { // compare raw bf16 bit pairs via float-diff of bits
      if (h0[i] != h1[i]) { ++diffs; if (first < 0) first = i; }
      continue;
    }
    if (d > 1e-4f * (fabsf(h0[i]) + 1.f)) {
      ++diffs;
      if (d > maxd) maxd = d;
      if (first < 0) first = i;
    }
  }
  bad = diffs != 0;
  printf("xcheck kind%d M%ld N%d K%d sk%d: %s (diffs %ld/%ld maxd %.4g "
         "first %ld)\n", kind, M, N, K, splits, bad ? "FAIL" : "OK", diffs,
         n_out, maxd, first);
  hipFree(da); hipFree(db); hipFree(dc0); hipFree(dc1);
  if (dacc0) hipFree(dacc0);
  return bad;
}

// ---- scalar vs 16-byte-store epilogue at the flagship's shapes (--epi) --
// kind 0: NT×NT through launch_nt_gemm (1x1 conv forward; the route — 256²
// or 128² pipe — is the library's own choice), kind 1: TN×TN (wgrad; the
// 3x3 wgrad's gather is replaced by plain operands of the same GEMM shape).
// Output bf16 when splits == 1, fp32 slabs otherwise, as in the model.
// Each figure is the mean of `iters` back-to-back launches; scalar and
// vector alternate over three rounds so drift shows as spread, not as gain.
static void bench_epi(const char *name, int kind, int M, int N, int K,
                      int splits, int iters) {
  uint16_t *da, *db;
  void *dc;
  bool f32 = splits > 1;
  CHECK(hipMalloc(&da, (long)M * K * 2));
  CHECK(hipMalloc(&db, (long)N * K * 2));
  CHECK(hipMalloc(&dc, (long)splits * M * N * (f32 ? 4 : 2)));
  CHECK(hipMemset(da, 0x3c, (long)M * K * 2));
  CHECK(hipMemset(db, 0x3c, (long)N * K * 2));
  auto launch = [&]() -> hipError_t {
    if (kind == 0) {
      GemmLoader la{da, M, (long)K, K};
      GemmLoader lb{db, N, (long)K, K};
      return launch_nt_gemm(la, lb, dc, M, N, K, N, f32, 0, splits);
    }
    TnPipe<PlainTnSrc> sa{{da, (long)M, K, M}};
    TnPipe<PlainTnSrc> sb{{db, (long)N, K, N}};
    return launch_pipe_mix_wr(sa, sb, dc, M, N, K, LinearWriter{(long)N}, N,
                              f32, 0, splits);
  };
  float us[2][3];
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int round = 0; round < 3; ++round)
    for (int vec = 0; vec < 2; ++vec) {
      g_epilogue_vec.store(vec != 0);
      CHECK(launch()); // warm-up, also loads the code object
      CHECK(hipDeviceSynchronize());
      hipEventRecord(e0);
      for (int i = 0; i < iters; ++i) launch();
      hipEventRecord(e1);
      CHECK(hipEventSynchronize(e1));
      float ms;
      hipEventElapsedTime(&ms, e0, e1);
      us[vec][round] = ms * 1e3f / iters;
    }
  hipEventDestroy(e0); hipEventDestroy(e1);
  g_epilogue_vec.store(true);
  printf("epi %-22s M%-6d N%-5d K%-6d sk%-2d %s  scalar %7.2f %7.2f %7.2f us"
         "  vector %7.2f %7.2f %7.2f us\n", name, M, N, K, splits,
         f32 ? "f32 " : "bf16", us[0][0], us[0][1], us[0][2], us[1][0],
         us[1][1], us[1][2]);
  hipFree(da); hipFree(db); hipFree(dc);
}

static int conv_splits_h(long M, int Ncols, int K) {
  long tiles = ((M + 127) / 128) * ((Ncols + 127) / 128);
  int nk = (K + 63) / 64;
  if (tiles >= 256 || nk < 16) return 1;
  long s = 512 / tiles;
  if (s > nk / 8) s = nk / 8;
  if (s > 16) s = 16;
  return s < 1 ? 1 : (int)s;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--probe")) {
    run_probe();
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--xcheck256")) {
    // pipe256 (new default <swz1,1bar,sprio>) vs gemm256 (round-1 oracle)
    // at the exact ResNet 1x1-fwd + BERT linear shapes that route there
    struct S { int M, N, K; } shapes[] = {
        {200704, 256, 64},  {200704, 64, 256},  {50176, 512, 128},
        {50176, 256, 512},  {12544, 1024, 256}, {12544, 512, 1024},
        {3136, 2048, 512},  {4096, 4096, 1024}, {4096, 1024, 4096},
    };
    int bad = 0;
    for (auto &sh : shapes) {
      long M = sh.M;
      int N = sh.N, K = sh.K;
      if (M % 256 || N % 256 || K % 32 || (M / 256) * (N / 256) < 128) {
        printf("x256 M%ld N%d K%d: skipped (not a 256-route shape)\n", M, N, K);
        continue;
      }
      uint16_t *da, *db;
      float *d0, *d1;
      CHECK(hipMalloc(&da, M * K * 2));
      CHECK(hipMalloc(&db, (long)N * K * 2));
      CHECK(hipMalloc(&d0, M * N * 4));
      CHECK(hipMalloc(&d1, M * N * 4));
      {
        std::vector<uint16_t> h(M * K);
        unsigned x = 0xbeef123u;
        for (auto &v : h) {
          x = x * 1664525u + 1013904223u;
          v = f2bf_h(((x >> 8) & 0xffff) / 32768.0f - 1.0f);
        }
        CHECK(hipMemcpy(da, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        h.resize((long)N * K);
        for (auto &v : h) {
          x = x * 1664525u + 1013904223u;
          v = f2bf_h(((x >> 8) & 0xffff) / 32768.0f - 1.0f);
        }
        CHECK(hipMemcpy(db, h.data(), h.size() * 2, hipMemcpyHostToDevice));
      }
      GemmLoader la{da, (int)M, (long)K, K};
      GemmLoader lb{db, N, (long)K, K};
      CHECK(launch_nt256(la, lb, d0, (int)M, N, K, N, true, 0));
      CHECK(hipDeviceSynchronize());
      CHECK(launch_pipe256(la, lb, d1, (int)M, N, K, N, true, 0));
      CHECK(hipDeviceSynchronize());
      std::vector<float> h0(M * N), h1(M * N);
      CHECK(hipMemcpy(h0.data(), d0, M * N * 4, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(h1.data(), d1, M * N * 4, hipMemcpyDeviceToHost));
      long diffs = 0, first = -1;
      float maxd = 0;
      for (long i = 0; i < M * N; ++i) {
        float d = fabsf(h0[i] - h1[i]);
        if (d > 1e-4f * (fabsf(h0[i]) + 1.f)) {
          ++diffs;
          if (d > maxd) maxd = d;
          if (first < 0) first = i;
        }
      }
      printf("x256 M%ld N%d K%d: %s (diffs %ld/%ld maxd %.4g first %ld "
             "row %ld col %ld)\n", M, N, K, diffs ? "FAIL" : "OK", diffs,
             M * N, maxd, first, first >= 0 ? first / N : -1,
             first >= 0 ? first % N : -1);
      bad += diffs != 0;
      hipFree(da); hipFree(db); hipFree(d0); hipFree(d1);
    }
    printf(bad ? "X256 FAILURES\n" : "x256 all OK\n");
    return bad != 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--xcheck")) {
    int bad = 0;
    // ResNet101 bs64 1x1 dgrad shapes (M=NHW, N=C, K=Kout) + model splits
    bad += xcheck(1, 200704, 64, 256, conv_splits_h(200704, 64, 256));
    bad += xcheck(1, 200704, 256, 64, conv_splits_h(200704, 256, 64));
    bad += xcheck(1, 50176, 128, 512, conv_splits_h(50176, 128, 512));
    bad += xcheck(1, 12544, 256, 1024, conv_splits_h(12544, 256, 1024));
    bad += xcheck(1, 3136, 512, 2048, conv_splits_h(3136, 512, 2048));
    // dgrad-acc (bottleneck conv1 accumulate)
    bad += xcheck(2, 50176, 256, 128, 1);
    bad += xcheck(2, 12544, 512, 256, 1);
    bad += xcheck(2, 3136, 1024, 512, 1);
    // 1x1 wgrad (TN×TN over pixel K) + FC backward
    bad += xcheck(0, 256, 64, 200704, 8);
    bad += xcheck(0, 512, 2048, 3136, 8);
    bad += xcheck(0, 1000, 2048, 64, 1);
    bad += xcheck(1, 64, 2048, 1000, 1);
    printf(bad ? "XCHECK FAILURES\n" : "xcheck all OK\n");
    return bad != 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--epi")) {
    // ResNet101 bs64 shapes (M, N, K as the GEMM sees them)
    bench_epi("layer3 conv3 fwd", 0, 12544, 1024, 256, 1, 200);
    bench_epi("layer3 conv1 fwd", 0, 12544, 256, 1024, 2, 200);
    bench_epi("layer3 conv1 wgrad", 1, 256, 1024, 12544, 24, 200);
    bench_epi("layer1 conv3 fwd", 0, 200704, 256, 64, 1, 100);
    bench_epi("layer3 3x3 wgrad", 1, 256, 2304, 12544, 8, 200);
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--tn-debug")) {
    run_tn_debug();
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--tn")) {
    int fails = 0;
    fails += check_tn(0, 256, 256, 64, 1);    // single-ish tiles, nk=1
    fails += check_tn(0, 384, 384, 192, 1);   // nk=3 pipeline
    fails += check_tn(0, 200, 72, 136, 1);    // ragged M/N (K%8)
    fails += check_tn(0, 256, 512, 777, 1);   // ragged K (TN granule=1 k)
    fails += check_tn(0, 256, 256, 2048, 4);  // split-K slabs
    fails += check_tn(1, 256, 256, 128, 1);   // NT×TN
    fails += check_tn(1, 300, 200, 512, 1);   // NT×TN ragged
    fails += check_tn(1, 256, 512, 1024, 4);  // NT×TN split-K
    if (fails) { printf("TN NUMERICS FAILURES: %d\n", fails); return 1; }
    // wgrad-class: dw[256][2304] over M=200k pixels (ResNet stage3 3x3
    // runs as gather; this is the same GEMM shape with plain operands);
    // 1x1 wgrad dw[512][2048]; linear dw/dx (BERT-Large bs32)
    // BERT dw split sweep: prologue share vs chip fill at kt = nk/splits
    bench_tn(0, 1024, 1024, 4096, 2, 25);
    bench_tn(0, 1024, 1024, 4096, 4, 25);
    bench_tn(0, 1024, 1024, 4096, 8, 25);
    bench_tn(0, 1024, 1024, 4096, 16, 25);
    bench_tn(0, 1024, 4096, 4096, 2, 25);
    bench_tn(0, 1024, 4096, 4096, 4, 25);
    bench_tn(0, 256, 2304, 200704, 8, 10);
    bench_tn(0, 512, 2048, 50176, 8, 10);
    bench_tn(0, 1024, 1024, 4096, 1, 25);
    bench_tn(0, 4096, 1024, 4096, 1, 25);
    bench_tn(1, 4096, 1024, 1024, 1, 25);
    bench_tn(1, 16384, 1024, 1024, 1, 25);
    bench_tn(1, 12544, 256, 1024, 1, 25);
    return 0;
  }
  int fails = 0;
  fails += check_small(256, 256, 64);   // single tile, nk=1 (drain path)
  fails += check_small(256, 256, 128);  // nk=2: prologue+steady+epilogue
  fails += check_small(512, 512, 192);  // multi-tile, nk=3
  fails += check_small(512, 256, 320);  // deeper pipeline, asymmetric grid
  if (fails) { printf("NUMERICS FAILURES: %d\n", fails); return 1; }
  bench(4096, 4096, 4096, 25);
  bench(8192, 8192, 8192, 8);
  // real model shapes on this path: ResNet stage-2/3 1x1 convs (M=NHW),
  // BERT-Large MLM head (vocab-padded 30720)
  bench(50176, 512, 256, 25);
  bench(12544, 1024, 512, 25);
  bench(4096, 30720, 1024, 12);
  return 0;
}
