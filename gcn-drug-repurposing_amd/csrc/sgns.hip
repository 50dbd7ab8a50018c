// sgns.hip -- skip-gram with negative sampling over the node2vec walks: gensim 3.x Word2Vec(sg=1, hs=0, negative, window, sample)
// as multiscale/openne/node2vec.py:7-38 calls it (word2vec_inner.pyx train_batch_sg / fast_sentence_sg_neg).
//
// Per sentence (one walk) and epoch: tokens are kept with gensim's downsampling rule (uint32 draw <= sample_int[word]), the kept
// tokens form the sentence; per kept position i (the center c) a reduced window b in [0, window) is drawn and every kept context
// x within window - b positions does one pair update:
//     l1 = syn0[x], neu1e = 0;  for t in [c] + negatives (a negative equal to c is skipped):
//         f = l1 . syn1neg[t];  if |f| < 6:  g = (label - sigmoid(f)) alpha;  neu1e += g syn1neg[t];  syn1neg[t] += g l1
//     syn0[x] += neu1e
// Sigmoid: evaluated exactly, 1 / (1 + expf(-f)) in fp32, with gensim's rule that skips the target when |f| >= MAX_EXP = 6
// (gensim reads a 1000-entry table instead; the mirror does what this kernel does).
// alpha = max(min_alpha, alpha0 - (alpha0 - min_alpha) (epoch + s / S) / epochs) for sentence s of S: a function of (epoch, s).
//
// Parallelism: `concurrency` persistent waves, wave k owns the contiguous sentence range [S k / C, S (k + 1) / C) and walks it
// in order, one center position at a time (Hogwild across waves, like gensim's worker threads on their jobs).  With C = 1 the
// whole epoch runs in the serial order of tests/node2vec_mirror.py.  Every row (the center's syn1neg row included) is loaded, updated
// and stored per pair, as gensim does: keeping the center's row in registers across a position's contexts would be serially exact too,
// but its final store overwrites the negative updates other waves made to that row meanwhile -- with thousands of waves in flight on a
// vocabulary of a few thousand nodes, most of them.  A row of d floats is d / 64 consecutive floats per lane; dot products are reduced across
// the wave with xor shuffles (fp32), so a serial run differs from the numpy mirror by that reduction order only.
// Draws (counter_rng.h): reduced window (seed, epoch, token), keep (seed, epoch, token), negative k of a pair (seed, epoch, center
// token, context token * 64 + k) -- tokens are indices into the walks array, so serial and Hogwild runs see one random stream.
#include "common.h"
#include "counter_rng.h"

namespace gss {
namespace {

constexpr int kWavesPerBlock = 4;
constexpr float kMaxExp = 6.f;

__global__ void token_count_kernel(int64_t n_walks, int32_t L, const int32_t *__restrict__ walks, const int32_t *__restrict__ lengths,
                                   unsigned long long *__restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_walks * L) return;
  const int64_t s = t / L;
  const int32_t pos = (int32_t)(t - s * L);
  if (pos < lengths[s]) atomicAdd(counts + walks[t], 1ull);
}

__global__ void sgns_init_kernel(int32_t n, int32_t d, uint64_t seed, float *__restrict__ syn0, float *__restrict__ syn1) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * d) return;
  const int64_t node = i / d, comp = i - node * d;
  const float u = rng_unit_f32(rng_key(seed, kRngInit, (uint64_t)node, (uint64_t)comp, 0));
  syn0[i] = __fdiv_rn(u - 0.5f, (float)d);
  syn1[i] = 0.f;
}

struct SgnsArgs {
  int32_t n, d, walk_length, window, negative, epochs, epoch;
  int64_t n_walks;
  const int32_t *walks, *lengths;
  const uint32_t *cum_table;
  const int64_t *sample_int;
  uint32_t cum_last;
  float alpha, min_alpha;
  uint64_t seed;
  int32_t concurrency;
  float *syn0, *syn1;
};

template <int VPL>
__device__ __forceinline__ float dotw(const float (&a)[VPL], const float (&b)[VPL]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < VPL; ++k) s = fmaf(a[k], b[k], s);
  return wave_sum(s);
}

// Rows are shared by every wave of the device: agent-scope (relaxed) accesses keep them coherent across the XCDs.  With plain accesses
// a row written on one XCD stays in that XCD's L2 and the others keep reading their own stale copy -- each XCD then trains a replica of
// its own and the rows come back as a mixture of their cache lines (measured: a 10-NN community purity of 0.13, chance level).
template <int VPL>
__device__ __forceinline__ void load_row(float (&r)[VPL], float *p) {
#pragma unroll
  for (int k = 0; k < VPL; ++k) r[k] = __hip_atomic_load(p + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int VPL>
__device__ __forceinline__ void store_row(float *p, const float (&r)[VPL]) {
#pragma unroll
  for (int k = 0; k < VPL; ++k) __hip_atomic_store(p + k, r[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float sigmoidf(float f) { return 1.f / (1.f + expf(-f)); }

template <int VPL>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void sgns_epoch_kernel(SgnsArgs a) {
  extern __shared__ int32_t lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = threadIdx.x / kWave;
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + wib;
  if (wave >= a.concurrency) return;
  const int32_t L = a.walk_length;
  int32_t *knode = lds + wib * 2 * L;  // kept tokens of the current sentence: node, position in the walk
  int32_t *kpos = knode + L;
  const int64_t S = a.n_walks;
  const int64_t s_begin = S * wave / a.concurrency, s_end = S * (wave + 1) / a.concurrency;
  const int off = lane * VPL;
  for (int64_t s = s_begin; s < s_end; ++s) {
    const double progress = ((double)a.epoch + (double)s / (double)S) / (double)a.epochs;
    const float alpha = (float)fmax((double)a.min_alpha, (double)a.alpha - ((double)a.alpha - (double)a.min_alpha) * progress);
    const int32_t len = a.lengths[s];
    const int64_t tok0 = s * L;
    // downsampling: the kept tokens, compacted in order into this wave's LDS slice
    int32_t klen = 0;
    for (int32_t base = 0; base < len; base += kWave) {
      const int32_t p = base + lane;
      bool keep = false;
      int32_t node = 0;
      if (p < len) {
        node = a.walks[tok0 + p];
        const uint32_t r = rng_u32(rng_key(a.seed, kRngKeep, (uint64_t)a.epoch, (uint64_t)(tok0 + p), 0));
        keep = (int64_t)r <= a.sample_int[node];
      }
      const uint64_t m = __ballot(keep);
      if (keep) {
        const int32_t k = klen + __popcll(m & ((1ull << lane) - 1ull));
        knode[k] = node;
        kpos[k] = p;
      }
      klen += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int32_t i = 0; i < klen; ++i) {
      const int32_t c = knode[i];
      const int64_t ti = tok0 + kpos[i];
      const int32_t b = (int32_t)(rng_u32(rng_key(a.seed, kRngWindow, (uint64_t)a.epoch, (uint64_t)ti, 0)) % (uint32_t)a.window);
      const int32_t lo = max(0, i - a.window + b), hi = min(klen, i + a.window + 1 - b);
      float *hrow = a.syn1 + (int64_t)c * a.d + off;
      for (int32_t j = lo; j < hi; ++j) {
        if (j == i) continue;
        const int32_t x = knode[j];
        const int64_t tj = tok0 + kpos[j];
        // lane k in [1, negative] draws negative k: bisect_left(cum_table, r % cum_table[-1])
        int32_t tgt = -1;
        if (lane >= 1 && lane <= a.negative) {
          const uint32_t r = rng_u32(rng_key(a.seed, kRngNeg, (uint64_t)a.epoch, (uint64_t)ti, (uint64_t)tj * 64 + (uint64_t)lane)) % a.cum_last;
          int32_t l = 0, u = a.n;
          while (l < u) {
            const int32_t mid = (l + u) >> 1;
            if (a.cum_table[mid] < r) l = mid + 1;
            else u = mid;
          }
          tgt = l;
        }
        float *xrow = a.syn0 + (int64_t)x * a.d + off;
        float l1[VPL], neu[VPL];
        load_row(l1, xrow);
#pragma unroll
        for (int k = 0; k < VPL; ++k) neu[k] = 0.f;
        {
          float h[VPL];
          load_row(h, hrow);
          const float f = dotw(l1, h);
          if (fabsf(f) < kMaxExp) {
            const float g = (1.f - sigmoidf(f)) * alpha;
#pragma unroll
            for (int k = 0; k < VPL; ++k) {
              neu[k] = fmaf(g, h[k], neu[k]);
              h[k] = fmaf(g, l1[k], h[k]);
            }
            store_row(hrow, h);
          }
        }
        for (int k = 1; k <= a.negative; ++k) {
          const int32_t t = __shfl(tgt, k, kWave);
          if (t == c) continue;
          float *trow = a.syn1 + (int64_t)t * a.d + off;
          float r[VPL];
          load_row(r, trow);
          const float f = dotw(l1, r);
          if (fabsf(f) >= kMaxExp) continue;
          const float g = (0.f - sigmoidf(f)) * alpha;
#pragma unroll
          for (int q = 0; q < VPL; ++q) {
            neu[q] = fmaf(g, r[q], neu[q]);
            r[q] = fmaf(g, l1[q], r[q]);
          }
          store_row(trow, r);
        }
        float cur[VPL];
        load_row(cur, xrow);  // Hogwild: add to the row as it is now (serially it is still l1)
#pragma unroll
        for (int k = 0; k < VPL; ++k) cur[k] += neu[k];
        store_row(xrow, cur);
      }
    }
    __builtin_amdgcn_wave_barrier();  // this sentence's LDS slice is read to the end before the next one overwrites it
  }
}

template <int VPL>
int launch_epoch(const SgnsArgs &a, hipStream_t st) {
  const size_t lds = (size_t)kWavesPerBlock * 2 * a.walk_length * sizeof(int32_t);
  const int blocks = ceil_div(a.concurrency, kWavesPerBlock);
  hipLaunchKernelGGL(sgns_epoch_kernel<VPL>, dim3(blocks), dim3(kWave * kWavesPerBlock), lds_request(sgns_epoch_kernel<VPL>, lds), st, a);
  GSS_LAUNCH_CHECK("sgns_epoch_kernel");
  return GSS_OK;
}

}  // namespace

extern "C" {

int gss_sgns_counts(int64_t n_walks, int32_t walk_length, const int32_t *walks, const int32_t *lengths, int64_t *counts, void *stream) {
  GSS_REQUIRE(walk_length >= 1 && n_walks >= 0, "sgns_counts: walk_length=%d, n_walks=%lld", walk_length, (long long)n_walks);
  GSS_REQUIRE(walks && lengths && counts, "sgns_counts: null pointer");
  const int64_t tokens = n_walks * walk_length;
  if (tokens == 0) return GSS_OK;
  const int64_t blocks = (tokens + 255) / 256;
  GSS_REQUIRE(blocks <= 0x7fffffff, "sgns_counts: %lld tokens are too many for one launch", (long long)tokens);
  token_count_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(n_walks, walk_length, walks, lengths,
                                                                      reinterpret_cast<unsigned long long *>(counts));
  GSS_LAUNCH_CHECK("token_count_kernel");
  return GSS_OK;
}

int gss_sgns_init(int32_t n, int32_t d, uint64_t seed, float *syn0, float *syn1neg, void *stream) {
  GSS_REQUIRE(n >= 1 && d >= 1, "sgns_init: n=%d d=%d", n, d);
  GSS_REQUIRE(syn0 && syn1neg, "sgns_init: null pointer");
  const int64_t total = (int64_t)n * d;
  const int64_t blocks = (total + 255) / 256;
  GSS_REQUIRE(blocks <= 0x7fffffff, "sgns_init: %lld values are too many for one launch", (long long)total);
  sgns_init_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(n, d, seed, syn0, syn1neg);
  GSS_LAUNCH_CHECK("sgns_init_kernel");
  return GSS_OK;
}

int gss_sgns_default_concurrency(void) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    return fail(GSS_EHIP, "sgns_default_concurrency: no device");
  return cus * 16;
}

int gss_sgns_epoch(const gss_sgns_desc *desc, int32_t epoch, float *syn0, float *syn1neg, void *stream) {
  GSS_REQUIRE(desc, "sgns_epoch: null descriptor");
  const gss_sgns_desc &D = *desc;
  GSS_REQUIRE(D.n >= 1, "sgns_epoch: n=%d must be >= 1", D.n);
  GSS_REQUIRE(D.d == 64 || D.d == 128 || D.d == 256 || D.d == 512, "sgns_epoch: dim=%d unsupported (64, 128, 256 or 512)", D.d);
  GSS_REQUIRE(D.walk_length >= 1 && D.walk_length <= 2048, "sgns_epoch: walk_length=%d must be in [1, 2048]", D.walk_length);
  GSS_REQUIRE(D.window >= 1, "sgns_epoch: window=%d must be >= 1", D.window);
  GSS_REQUIRE(D.negative >= 1 && D.negative <= 63, "sgns_epoch: negative=%d must be in [1, 63]", D.negative);
  GSS_REQUIRE(D.epochs >= 1 && epoch >= 0 && epoch < D.epochs, "sgns_epoch: epoch=%d of epochs=%d", epoch, D.epochs);
  GSS_REQUIRE(D.concurrency >= 1, "sgns_epoch: concurrency=%d must be >= 1", D.concurrency);
  GSS_REQUIRE(D.n_walks >= 0, "sgns_epoch: n_walks=%lld", (long long)D.n_walks);
  GSS_REQUIRE(D.walks && D.lengths && D.cum_table && D.sample_int && syn0 && syn1neg, "sgns_epoch: null pointer");
  GSS_REQUIRE(D.cum_last >= 1, "sgns_epoch: cum_last=%u must be >= 1 (the last entry of cum_table)", D.cum_last);
  if (D.n_walks == 0) return GSS_OK;
  SgnsArgs a;
  a.n = D.n;
  a.d = D.d;
  a.walk_length = D.walk_length;
  a.window = D.window;
  a.negative = D.negative;
  a.epochs = D.epochs;
  a.epoch = epoch;
  a.n_walks = D.n_walks;
  a.walks = D.walks;
  a.lengths = D.lengths;
  a.cum_table = D.cum_table;
  a.sample_int = D.sample_int;
  a.cum_last = D.cum_last;
  a.alpha = D.alpha;
  a.min_alpha = D.min_alpha;
  a.seed = D.seed;
  a.concurrency = (int32_t)(D.concurrency < D.n_walks ? D.concurrency : D.n_walks);
  a.syn0 = syn0;
  a.syn1 = syn1neg;
  hipStream_t st = as_stream(stream);
  switch (D.d) {
    case 64: return launch_epoch<1>(a, st);
    case 128: return launch_epoch<2>(a, st);
    case 256: return launch_epoch<4>(a, st);
    default: return launch_epoch<8>(a, st);
  }
}

}  // extern "C"
}  // namespace gss
