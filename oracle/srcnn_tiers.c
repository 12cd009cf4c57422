/*
 * srcnn_tiers.c -- CPU restatement of the PRODUCT's fp32 non-parity tiers (SRCNN_MODE_RELAXED bits, SRCNN_MODE_FAST).
 *
 * TEST INFRASTRUCTURE ONLY, like srcnn_oracle.c, and apart from it on purpose: srcnn_oracle.c restates the REFERENCE; this
 * file restates the arithmetic the product itself states for its relaxations (include/srcnn_amd_debug.h, DESIGN.md 3, the
 * RELAX / X64 branches and k_conv3_fast of libsrcnn_amd/csrc/srcnn_kernels.hip), so that those tiers can be held to
 * tolerance 0 as well (tests/test_gpu_tiers_exact.py).  The product never links it.
 *
 * With every relaxation off each function is srcnn_oracle.c's, operation for operation (the tests pin that bit for bit):
 * same padding (clamp to edge), same tap, channel and weight order, same ReLU and clamp.  A relaxation replaces exactly the
 * operations named below and nothing else:
 *   layer 1, fma      : acc = fmaf(w1[k][t], y[t], acc) over the 81 taps, from 0     (v_mfma_f32_32x32x1, C = acc)
 *   layer 2, K=2 model: acc2 = step(acc2, pair p) over the channel pairs (2p, 2p+1)  (v_mfma_f32_32x32x2f32, C = acc2)
 *                         A  fmaf(w1, x1, fmaf(w0, x0, acc))      the pair in order, one rounding per channel
 *                         B  fmaf(w0, x0, fmaf(w1, x1, acc))      the pair reversed
 *                         C  round(acc + w0 x0 + w1 x1)           one rounding per pair
 *   layer 3, x64      : a = fma((double)w, (double)v, a) in window order; sum = (float)((double)sum + a)
 *   layer 3, f32      : a = fmaf(w, v, a) in window order from 0; sum = sum + a in fp32
 * Build with -ffp-contract=off: every fused operation here is an explicit fmaf / fma call, everything else rounds on its own.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define C1 64
#define C2 32

static const uint32_t k_weight_bits[8129] = {
#include "oracle_weights.inc"
};

#define OFF_B1 0
#define OFF_W1 (OFF_B1 + 64)
#define OFF_B2 (OFF_W1 + 64 * 81)
#define OFF_W2 (OFF_B2 + 32)
#define OFF_B3 (OFF_W2 + 32 * 64)
#define OFF_W3 (OFF_B3 + 1)

static inline const float* wtab(void) { return (const float*)(const void*)k_weight_bits; }
static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

enum { K2_STRICT = 0, K2_A = 1, K2_B = 2, K2_C = 3 };
enum { L3_STRICT = 0, L3_X64 = 1, L3_F32 = 2 };

/* layer 1.  fma = 0: the reference's product-then-add;  fma != 0: SRCNN_RELAX_L1.  out: 64 planes of w*h. */
void tiers_conv1(const float* y, unsigned w, unsigned h, int fma, float* out)
{
    const float* W = wtab() + OFF_W1;
    const float* B = wtab() + OFF_B1;
    const unsigned pw = w + 8, ph = h + 8;
    float* pad = (float*)malloc(sizeof(float) * (size_t)pw * ph);
    for (unsigned r = 0; r < ph; ++r)
        for (unsigned c = 0; c < pw; ++c)
            pad[(size_t)r * pw + c] =
                y[(size_t)clampi((int)r - 4, 0, (int)h - 1) * w + clampi((int)c - 4, 0, (int)w - 1)];
#pragma omp parallel for
    for (int k = 0; k < C1; ++k) {
        const float* ker = W + k * 81;
        float* dst = out + (size_t)k * w * h;
        for (unsigned r = 0; r < h; ++r)
            for (unsigned c = 0; c < w; ++c) {
                float acc = 0;
                for (int i = 0; i < 9; ++i)
                    for (int j = 0; j < 9; ++j) {
                        const float wt = ker[i * 9 + j], v = pad[(size_t)(r + i) * pw + (c + j)];
                        if (fma) acc = fmaf(wt, v, acc);
                        else acc += wt * v;
                    }
                acc += B[k];
                dst[(size_t)r * w + c] = (acc >= 0) ? acc : 0;
            }
    }
    free(pad);
}

/* one K=2 step of layer 2 on the pair (w0, x0), (w1, x1) */
static inline float k2_step(int model, float acc, float w0, float x0, float w1, float x1)
{
    switch (model) {
    case K2_A: return fmaf(w1, x1, fmaf(w0, x0, acc));
    case K2_B: return fmaf(w0, x0, fmaf(w1, x1, acc));
    case K2_C: {
        /* fp32 x fp32 is exact in fp64 (48 bits); the three-term sum is exact in binary128 unless the terms lie more than
         * 2^64 apart, where the smallest cannot reach the fp32 rounding of the result */
        const double p0 = (double)w0 * (double)x0, p1 = (double)w1 * (double)x1;
        return (float)((__float128)acc + (__float128)p0 + (__float128)p1);
    }
    default: acc += x0 * w0; acc += x1 * w1; return acc;
    }
}

/* layer 2.  model = K2_STRICT: the reference;  K2_A / _B / _C: SRCNN_RELAX_L2 under that model.  in: 64 planes, out: 32. */
void tiers_conv2(const float* in, unsigned w, unsigned h, int model, float* out)
{
    const float* W = wtab() + OFF_W2;
    const float* B = wtab() + OFF_B2;
    const size_t n = (size_t)w * h;
#pragma omp parallel for
    for (int m = 0; m < C2; ++m) {
        const float* ker = W + m * C1;
        float* dst = out + (size_t)m * n;
        for (size_t p = 0; p < n; ++p) {
            float acc = 0;
            for (int f = 0; f < C1; f += 2)
                acc = k2_step(model, acc, ker[f], in[(size_t)f * n + p], ker[f + 1], in[(size_t)(f + 1) * n + p]);
            acc += B[m];
            dst[p] = (acc >= 0) ? acc : 0;
        }
    }
}

/* layer 3.  kind = L3_STRICT: the reference;  L3_X64: SRCNN_RELAX_L3_X64;  L3_F32: SRCNN_RELAX_L3_F32.  in: 32 planes. */
void tiers_conv3(const float* in, unsigned w, unsigned h, int kind, float* out)
{
    const float* W = wtab() + OFF_W3;
    const float bias = wtab()[OFF_B3];
    const unsigned pw = w + 4, ph = h + 4;
    const size_t n = (size_t)w * h, pn = (size_t)pw * ph;
    float* pad = (float*)malloc(sizeof(float) * pn * C2);
#pragma omp parallel for
    for (int m = 0; m < C2; ++m)
        for (unsigned r = 0; r < ph; ++r)
            for (unsigned c = 0; c < pw; ++c)
                pad[m * pn + (size_t)r * pw + c] =
                    in[m * n + (size_t)clampi((int)r - 2, 0, (int)h - 1) * w +
                       clampi((int)c - 2, 0, (int)w - 1)];
#pragma omp parallel for
    for (long r = 0; r < (long)h; ++r)
        for (unsigned c = 0; c < w; ++c) {
            float sum = 0;
            for (int m = 0; m < C2; ++m) {
                double acc = 0;
                float accf = 0;
                for (int dy = 0; dy < 5; ++dy)
                    for (int dx = 0; dx < 5; ++dx) { /* weight index is [chan][col][row], as the reference's */
                        const float wt = W[m * 25 + dx * 5 + dy], v = pad[m * pn + (size_t)(r + dy) * pw + (c + dx)];
                        if (kind == L3_X64) acc = fma((double)wt, (double)v, acc);
                        else if (kind == L3_F32) accf = fmaf(wt, v, accf);
                        else acc += wt * v;
                    }
                if (kind == L3_F32) sum += accf;
                else sum += acc; /* (float)((double)sum + acc) */
            }
            sum += bias;
            sum = sum > 0.f ? sum : 0.f;
            sum = sum < 255.f ? sum : 255.f;
            out[(size_t)r * w + c] = sum;
        }
    free(pad);
}

/*
 * The three layers on an already resampled plane (the resampler is strict in every tier: oracle_resample).
 * mask: SRCNN_RELAX_* bits (1 layer 1, 2 layer 2 under `model`, 4 layer 3 x64, 8 layer 3 f32).  Returns 0, or -1.
 */
int tiers_layers(const float* up, unsigned w, unsigned h, unsigned mask, int model, float* out)
{
    if ((mask & ~0xfu) || ((mask & 4u) && (mask & 8u)) || model < K2_A || model > K2_C) return -1;
    const size_t n = (size_t)w * h;
    float* c1 = (float*)malloc(sizeof(float) * n * C1);
    float* c2 = (float*)malloc(sizeof(float) * n * C2);
    int rc = -1;
    if (c1 && c2) {
        tiers_conv1(up, w, h, (mask & 1u) != 0, c1);
        tiers_conv2(c1, w, h, (mask & 2u) ? model : K2_STRICT, c2);
        tiers_conv3(c2, w, h, (mask & 4u) ? L3_X64 : (mask & 8u) ? L3_F32 : L3_STRICT, out);
        rc = 0;
    }
    free(c1);
    free(c2);
    return rc;
}
