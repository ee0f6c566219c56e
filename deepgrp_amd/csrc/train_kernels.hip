// Training step of the GRU model (deepgrp/model.py:293-336 with Keras' CategoricalCrossentropy): forward over a batch of windows
// given by start positions, head (attention, dense, softmax, loss, d loss / d logits), backward through time over both directions,
// and the weight gradients.  DESIGN.md ("Training kernels") states the layout of the saved activations and the reduction order.
//
// Every sum that crosses threads runs in a fixed order (wave butterflies, LDS trees, sequential loops over partial results): no
// floating-point atomics, so one call gives the same bytes every time.
//
// The three recurrent products run on the matrix cores in fp32 (v_mfma_f32_16x16x4_f32: a k-ordered fp32 fma chain):
//   forward   hm[16, 3Up]  = h[16, Up] . U[Up, 3Up]            per step and tile of 16 windows
//   backward  dh[16, Up]  += dG[16, 3Up] . U^T[3Up, Up]         per step and tile
//   gradient  dU[Up, 3Up]  = sum over rows of h_prev^T . dG      over all B.T rows of a direction, split into fixed chunks
#include "dgrp_common.h"

#include <algorithm>
#include <mutex>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TR_MAXC = 16;
constexpr int TR_TCHUNK = 32;        // steps per partial of the kernel / bias column sums
constexpr int TR_HCHUNK = 32;        // the head's sums over the steps of a window: blocks of 32 terms, then the blocks (error ~ sqrt(32) +
                                     // sqrt(T / 32) roundings, not sqrt(T): 1300 terms in one chain cost 1e-6 of FF/kernel's gradient)

struct train_params {
    int T, u, Up, C, att, F;         // F = rows of FF/kernel (2u with attention)
    int64_t B, n;
    int nt;                          // tiles of 16 windows
    int ntc;                         // ceil(T / TR_TCHUNK)
    int nh;                          // floats of one window's head partial
    int total;                       // parameters
    int nthr;                        // block width of the forward and backward kernels (256 up to 64 padded units, else 512)
    int oK, oU, oB, oS, oFk, oFb;    // offsets into the flat parameter buffer
    const float *w;                  // flat parameters
    const uint8_t *idx;
    const int8_t *truth;             // [C, n]
    const int64_t *starts;           // [B]
    const float *masks;              // [B, 2, 5] or null
    float *Upad, *UTpad, *S, *AVG, *DAVG, *DL, *PH, *LOSSP, *PU, *PW;
    float *loss, *grads;
};

// The jobs of one launch chain, passed by value in the kernel arguments (8 x 224 bytes): blockIdx.z is the job.  Every kernel
// takes its own job's parameters and runs the one-job body; grid, block width and dynamic LDS are the largest of the jobs, and
// a workgroup or thread outside its own job's extent returns before the first barrier.
struct train_table {
    train_params job[DGRP_TRAIN_MAX_JOBS];
};

__device__ __forceinline__ int64_t tr_start(const train_params &p, int64_t b)
{
    if (b >= p.B) b = p.B - 1;
    int64_t s = p.starts[b];
    const int64_t hi = p.n - p.T;
    return s < 0 ? 0 : (s > hi ? hi : s);
}

// input channel of window start `s` at step t of direction dir (1: the reverse complement read backwards)
__device__ __forceinline__ int tr_channel(const train_params &p, int64_t s, int t, int dir)
{
    int c = p.idx[s + (dir ? p.T - 1 - t : t)];
    if (c > 4) c = 4;
    return dir ? (c < 4 ? 3 - c : 4) : c;
}

__device__ __forceinline__ float tr_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ int64_t tr_slot(const train_params &p, int dir, int tile, int t, int q)
{
    return ((((int64_t)dir * p.nt + tile) * p.T + t) * 5 + q) * 16 * p.Up;
}

__global__ void train_pack_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    const int Up = p.Up, u = p.u;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Up * 3 * Up) return;
    const int i = e / (3 * Up), col = e % (3 * Up), g = col / Up, j = col % Up;
    const float v = (i < u && j < u) ? p.w[p.oU + i * 3 * u + g * u + j] : 0.0f;
    p.Upad[e] = v;
    p.UTpad[(int64_t)col * Up + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (nt, 2), one workgroup per tile of 16 windows and direction.  LDS: h [16][Up + 4], hm [16][3Up], kernel [5][3u], bias [2][3u],
// masks [16][5], starts [16], channels [16].
__global__ void train_forward_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    extern __shared__ __align__(16) unsigned char tr_lds[];
    const int Up = p.Up, u = p.u, T = p.T, HS = Up + 4, G3 = 3 * Up;
    const int tile = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x, NT = p.nthr;
    const int lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
    if (tile >= p.nt || tid >= NT) return;
    int64_t *st = (int64_t *)tr_lds;
    float *h = (float *)(st + 16);
    float *hm = h + 16 * HS;
    float *Wl = hm + 16 * G3;
    float *bl = Wl + 15 * u;
    float *ml = bl + 6 * u;
    int *ch = (int *)(ml + 80);

    for (int e = tid; e < 16 * HS; e += NT) h[e] = 0.0f;
    for (int e = tid; e < 15 * u; e += NT) Wl[e] = p.w[p.oK + e];
    for (int e = tid; e < 6 * u; e += NT) bl[e] = p.w[p.oB + e];
    if (tid < 16) st[tid] = tr_start(p, (int64_t)tile * 16 + tid);
    if (tid < 80) {
        int64_t b = (int64_t)tile * 16 + tid / 5;
        if (b >= p.B) b = p.B - 1;
        ml[tid] = p.masks ? p.masks[(b * 2 + dir) * 5 + tid % 5] : 1.0f;
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        if (tid < 16) ch[tid] = tr_channel(p, st[tid], t, dir);
        for (int ct = wave; ct < G3 / 16; ct += nwave) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const float *ap = h + (lane & 15) * HS + (lane >> 4);
            const float *bp = p.Upad + (int64_t)(lane >> 4) * G3 + ct * 16 + (lane & 15);
            for (int k0 = 0; k0 < Up; k0 += 8) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0], bp[(int64_t)k0 * G3], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0 + 4], bp[(int64_t)(k0 + 4) * G3], acc1, 0, 0, 0);
            }
            for (int i = 0; i < 4; ++i) hm[(4 * (lane >> 4) + i) * G3 + ct * 16 + (lane & 15)] = acc0[i] + acc1[i];
        }
        __syncthreads();
        const int64_t sb = tr_slot(p, dir, tile, t, 0);
        for (int e = tid; e < 16 * Up; e += NT) {
            const int row = e / Up, j = e % Up;
            float z = 0.f, r = 0.f, hh = 0.f, hmh = 0.f, hn = 0.f;
            if (j < u) {
                const int c = ch[row];
                const float m = ml[row * 5 + c];
                const float *wr = Wl + c * 3 * u;
                const float *hr = hm + row * G3;
                z = tr_sigmoid((wr[j] * m + bl[j]) + (hr[j] + bl[3 * u + j]));
                r = tr_sigmoid((wr[u + j] * m + bl[u + j]) + (hr[Up + j] + bl[4 * u + j]));
                hmh = hr[2 * Up + j] + bl[5 * u + j];
                hh = tanhf((wr[2 * u + j] * m + bl[2 * u + j]) + r * hmh);
                hn = z * h[row * HS + j] + (1.0f - z) * hh;
                h[row * HS + j] = hn;
            }
            const int64_t step = (int64_t)16 * Up;
            p.S[sb + e] = hn;
            p.S[sb + step + e] = z;
            p.S[sb + 2 * step + e] = r;
            p.S[sb + 3 * step + e] = hh;
            p.S[sb + 4 * step + e] = hmh;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------- head
__device__ __forceinline__ float tr_wave_sum(float v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ float tr_block_sum(float v, float *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ float tr_block_max(float v, float *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// one workgroup of 256 threads per window.  LDS: Wff [F][C], bff [16], q / ctx / dctx [u] each, cl [16], sdl [16], a [T], da [T],
// red [256], part [256][C + 2].
__global__ void train_head_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    extern __shared__ __align__(16) unsigned char tr_lds[];
    const int u = p.u, Up = p.Up, T = p.T, C = p.C, F = p.F, att = p.att, off = att ? u : 0;
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
    const int64_t b = blockIdx.x;
    if (b >= p.B) return;
    const int tile = (int)(b >> 4), row = (int)(b & 15);
    float *Wff = (float *)tr_lds;
    float *bff = Wff + F * C;
    float *q = bff + 16;
    float *ctx = q + u;
    float *dctx = ctx + u;
    float *cl = dctx + u;
    float *sdl = cl + 16;
    float *a = sdl + 16;
    float *da = a + T;
    float *red = da + T;
    float *part = red + 256;
    const float *scale = p.w + p.oS;
    float *avg = p.AVG + b * T * u;
    float *davg = p.DAVG + b * T * u;
    float *dl = p.DL + b * T * C;
    const int64_t start = tr_start(p, b);

    for (int e = tid; e < F * C; e += NT) Wff[e] = p.w[p.oFk + e];
    if (tid < 16) bff[tid] = tid < C ? p.w[p.oFb + tid] : 0.0f;
    for (int e = tid; e < T * u; e += NT) {
        const int t = e / u, j = e % u;
        const float hf = p.S[tr_slot(p, 0, tile, t, 0) + row * Up + j];
        const float hr = p.S[tr_slot(p, 1, tile, t, 0) + row * Up + j];
        avg[e] = 0.5f * (hf + hr);
    }
    __syncthreads();
    if (att) {
        if (tid < u) q[tid] = avg[(int64_t)(T - 1) * u + tid];     // the average of the two final states IS avg[T - 1]
        __syncthreads();
        for (int t = wave; t < T; t += nwave) {
            float e = 0.0f;
            for (int j = lane; j < u; j += 64) e += scale[j] * tanhf(q[j] + avg[(int64_t)t * u + j]);
            e = tr_wave_sum(e);
            if (lane == 0) a[t] = e;
        }
        __syncthreads();
        float mx = -INFINITY;
        for (int t = tid; t < T; t += NT) mx = fmaxf(mx, a[t]);
        mx = tr_block_max(mx, red);
        float s = 0.0f;
        for (int t = tid; t < T; t += NT) {
            const float v = expf(a[t] - mx);
            a[t] = v;
            s += v;
        }
        s = tr_block_sum(s, red);
        for (int t = tid; t < T; t += NT) a[t] = a[t] / s;
        __syncthreads();
        if (tid < u) {
            float c = 0.0f;
            for (int t0 = 0; t0 < T; t0 += TR_HCHUNK) {
                const int t1 = min(T, t0 + TR_HCHUNK);
                float blk = 0.0f;
                for (int t = t0; t < t1; ++t) blk += a[t] * avg[(int64_t)t * u + tid];
                c += blk;
            }
            ctx[tid] = c;
        }
        __syncthreads();
    }
    if (tid < 16) {
        float c = bff[tid];
        if (att && tid < C)
            for (int j = 0; j < u; ++j) c += ctx[j] * Wff[j * C + tid];
        cl[tid] = c;
    }
    __syncthreads();

    // logits, softmax, loss and d loss / d logits: one wave per step
    const float inv_bt = 1.0f / ((float)p.B * (float)T);
    float lw = 0.0f;
    for (int t = wave; t < T; t += nwave) {
        float acc[TR_MAXC];
        for (int c = 0; c < TR_MAXC; ++c) acc[c] = 0.0f;
        for (int j = lane; j < u; j += 64) {
            const float v = avg[(int64_t)t * u + j];
            const float *wr = Wff + (off + j) * C;
            for (int c = 0; c < TR_MAXC; ++c)
                if (c < C) acc[c] += v * wr[c];
        }
        float mx = -INFINITY;
        for (int c = 0; c < TR_MAXC; ++c)
            if (c < C) {
                acc[c] = tr_wave_sum(acc[c]) + cl[c];
                mx = fmaxf(mx, acc[c]);
            }
        float s = 0.0f;
        for (int c = 0; c < TR_MAXC; ++c)
            if (c < C) {
                acc[c] = expf(acc[c] - mx);
                s += acc[c];
            }
        float s2 = 0.0f;
        for (int c = 0; c < TR_MAXC; ++c)
            if (c < C) {
                acc[c] = acc[c] / s;
                s2 += acc[c];
            }
        // Keras: probabilities divided by their sum, clipped to [1e-7, 1 - 1e-7]; a clipped term has no gradient
        float ysum = 0.0f, mine = 0.0f, pmine = 0.0f;
        for (int c = 0; c < TR_MAXC; ++c)
            if (c < C) {
                const float y = (float)p.truth[(int64_t)c * p.n + start + t];
                const float pn = acc[c] / s2;
                const bool inside = pn > 1e-7f && pn < 1.0f - 1e-7f;
                const float pc = fminf(fmaxf(pn, 1e-7f), 1.0f - 1e-7f);
                lw -= y * logf(pc);
                const float ye = inside ? y : 0.0f;
                ysum += ye;
                if (lane == c) {
                    mine = ye;
                    pmine = pn;
                }
            }
        if (lane < C) dl[(int64_t)t * C + lane] = (pmine * ysum - mine) * inv_bt;
    }
    lw = tr_block_sum(lane == 0 ? lw : 0.0f, red);
    if (tid == 0) p.LOSSP[b] = lw;
    if (!p.grads) return;
    __syncthreads();

    // column sums of d loss / d logits: one wave per class, a lane adds every 64th step, then the butterfly
    for (int c = wave; c < 16; c += nwave) {
        float s = 0.0f;
        if (c < C)
            for (int t = lane; t < T; t += 64) s += dl[(int64_t)t * C + c];
        s = tr_wave_sum(s);
        if (lane == 0) sdl[c] = s;
    }
    __syncthreads();
    if (att) {
        if (tid < u) {
            float d = 0.0f;
            for (int c = 0; c < C; ++c) d += Wff[tid * C + c] * sdl[c];
            dctx[tid] = d;
        }
        __syncthreads();
        for (int t = wave; t < T; t += nwave) {
            float d = 0.0f;
            for (int j = lane; j < u; j += 64) d += dctx[j] * avg[(int64_t)t * u + j];
            d = tr_wave_sum(d);
            if (lane == 0) da[t] = d;
        }
        __syncthreads();
        float dot = 0.0f;
        for (int t = tid; t < T; t += NT) dot += a[t] * da[t];
        dot = tr_block_sum(dot, red);
        for (int t = tid; t < T; t += NT) da[t] = a[t] * (da[t] - dot);      // d loss / d e[t]
        __syncthreads();
    }
    // thread (g, j): the steps t = g, g + G, ... of unit j; the G partial sums are added in the order of g afterwards
    const int G = NT / u, PS = C + 2;
    if (tid < G * u) {
        const int g = tid / u, j = tid % u;
        float wrow[TR_MAXC], accw[TR_MAXC], blkw[TR_MAXC];
        for (int c = 0; c < TR_MAXC; ++c) {
            wrow[c] = c < C ? Wff[(off + j) * C + c] : 0.0f;
            accw[c] = 0.0f;
            blkw[c] = 0.0f;
        }
        float dsc = 0.0f, dq = 0.0f, bsc = 0.0f, bq = 0.0f;
        const float sj = att ? scale[j] : 0.0f, qj = att ? q[j] : 0.0f, dcj = att ? dctx[j] : 0.0f;
        int k = 0;
        for (int t = g; t < T; t += G) {
            const float av = avg[(int64_t)t * u + j];
            float dv = 0.0f;
            for (int c = 0; c < TR_MAXC; ++c)
                if (c < C) {
                    const float d = dl[(int64_t)t * C + c];
                    dv += d * wrow[c];
                    blkw[c] += av * d;
                }
            if (att) {
                const float th = tanhf(qj + av), de = da[t];
                bsc += de * th;
                const float dp = de * sj * (1.0f - th * th);
                bq += dp;
                dv += a[t] * dcj + dp;
            }
            davg[(int64_t)t * u + j] = dv;
            if (++k == TR_HCHUNK || t + G >= T) {                 // a block of the thread's steps is complete: add it to the total
                for (int c = 0; c < TR_MAXC; ++c) {
                    accw[c] += blkw[c];
                    blkw[c] = 0.0f;
                }
                dsc += bsc;
                dq += bq;
                bsc = bq = 0.0f;
                k = 0;
            }
        }
        for (int c = 0; c < TR_MAXC; ++c)
            if (c < C) part[tid * PS + c] = accw[c];
        part[tid * PS + C] = dsc;
        part[tid * PS + C + 1] = dq;
    }
    __syncthreads();
    float *ph = p.PH + b * p.nh;
    if (tid < u) {
        const int j = tid;
        for (int c = 0; c < C + 2; ++c) {
            float s = 0.0f;
            for (int g = 0; g < G; ++g) s += part[(g * u + j) * PS + c];
            if (c < C) ph[off + (off + j) * C + c] = s;
            else if (att && c == C) ph[j] = s;
            else if (att) davg[(int64_t)(T - 1) * u + j] += s;                 // the query's gradient lands on avg[T - 1]
        }
        if (att)
            for (int c = 0; c < C; ++c) ph[u + j * C + c] = ctx[j] * sdl[c];
    }
    if (tid < C) ph[off + F * C + tid] = sdl[tid];
}

// --------------------------------------------------------------------------------------------------------------- backward
// grid (nt, 2).  LDS: dh [16][Up + 4], dg [16][3Up + 4].  The gate gradients overwrite the saved gates: z <- d a_z, r <- d a_r,
// hh <- d a_h . r (recurrent side), hmh <- d a_h (input side).
__global__ void train_backward_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    extern __shared__ __align__(16) unsigned char tr_lds[];
    const int Up = p.Up, u = p.u, T = p.T, HS = Up + 4, G3 = 3 * Up, GS = G3 + 4;
    const int tile = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x, NT = p.nthr;
    const int lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
    if (!p.grads || tile >= p.nt || tid >= NT) return;
    float *dh = (float *)tr_lds;
    float *dg = dh + 16 * HS;
    for (int e = tid; e < 16 * HS; e += NT) dh[e] = 0.0f;
    for (int e = tid; e < 16 * GS; e += NT) dg[e] = 0.0f;
    __syncthreads();
    const int64_t step = (int64_t)16 * Up;
    for (int t = T - 1; t >= 0; --t) {
        const int64_t sb = tr_slot(p, dir, tile, t, 0);
        for (int e = tid; e < 16 * Up; e += NT) {
            const int row = e / Up, j = e % Up;
            if (j >= u) continue;
            const int64_t b = (int64_t)tile * 16 + row;
            const float dav = b < p.B ? 0.5f * p.DAVG[(b * T + t) * u + j] : 0.0f;
            const float dht = dh[row * HS + j] + dav;
            const float z = p.S[sb + step + e], r = p.S[sb + 2 * step + e], hh = p.S[sb + 3 * step + e], hmh = p.S[sb + 4 * step + e];
            const float hp = t > 0 ? p.S[sb - 5 * step + e] : 0.0f;
            const float dah = dht * (1.0f - z) * (1.0f - hh * hh);
            const float daz = dht * (hp - hh) * z * (1.0f - z);
            const float dar = dah * hmh * r * (1.0f - r);
            const float dhr = dah * r;
            p.S[sb + step + e] = daz;
            p.S[sb + 2 * step + e] = dar;
            p.S[sb + 3 * step + e] = dhr;
            p.S[sb + 4 * step + e] = dah;
            dg[row * GS + j] = daz;
            dg[row * GS + Up + j] = dar;
            dg[row * GS + 2 * Up + j] = dhr;
            dh[row * HS + j] = dht * z;
        }
        __syncthreads();
        if (t > 0) {
            for (int ct = wave; ct < Up / 16; ct += nwave) {
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                const float *ap = dg + (lane & 15) * GS + (lane >> 4);
                const float *bp = p.UTpad + (int64_t)(lane >> 4) * Up + ct * 16 + (lane & 15);
                for (int k0 = 0; k0 < G3; k0 += 8) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0], bp[(int64_t)k0 * Up], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0 + 4], bp[(int64_t)(k0 + 4) * Up], acc1, 0, 0, 0);
                }
                for (int i = 0; i < 4; ++i) dh[(4 * (lane >> 4) + i) * HS + ct * 16 + (lane & 15)] += acc0[i] + acc1[i];
            }
        }
        __syncthreads();
    }
}

// dU partials: grid (ceil(tiles / 4), 2 nt), 4 waves, one 16 x 16 output tile per wave, K = the 16 (T - 1) rows of a chunk
__global__ void train_wgrad_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    const int Up = p.Up, T = p.T, G3 = 3 * Up, ntn = G3 / 16, ntile = (Up / 16) * ntn;
    const int lane = threadIdx.x & 63, id = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (!p.grads || id >= ntile || (int)blockIdx.y >= 2 * p.nt) return;
    const int chunk = blockIdx.y, mi = id / ntn, ni = id % ntn, g = (ni * 16) / Up, nc = (ni * 16) % Up;
    const int64_t step = (int64_t)16 * Up, base = (int64_t)chunk * T * 5 * step;
    f32x4 acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int la = (lane >> 4) * Up + mi * 16 + (lane & 15), lb = (lane >> 4) * Up + nc + (lane & 15);
    for (int t = 1; t < T; ++t) {
        const float *hb = p.S + base + (int64_t)(t - 1) * 5 * step + la;
        const float *gb = p.S + base + ((int64_t)t * 5 + 1 + g) * step + lb;
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(hb[4 * i * Up], gb[4 * i * Up], acc[i], 0, 0, 0);
    }
    float *out = p.PU + (int64_t)chunk * Up * G3;
    for (int i = 0; i < 4; ++i)
        out[(int64_t)(mi * 16 + 4 * (lane >> 4) + i) * G3 + ni * 16 + (lane & 15)] = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
}

// kernel and bias partials: grid (2 nt, ntc), 3Up threads: thread n owns column n of the chunk's gate gradients
__global__ void train_colsum_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    const int Up = p.Up, T = p.T, G3 = 3 * Up, n = threadIdx.x;
    if (!p.grads || n >= G3 || (int)blockIdx.x >= 2 * p.nt || (int)blockIdx.y >= p.ntc) return;
    const int chunk = blockIdx.x, tc = blockIdx.y, dir = chunk / p.nt, tile = chunk % p.nt;
    const int g = n / Up, j = n % Up;
    const int64_t step = (int64_t)16 * Up, base = (int64_t)chunk * T * 5 * step;
    float w[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, bx = 0.0f, bh = 0.0f;
    const int t1 = min(T, (tc + 1) * TR_TCHUNK);
    for (int row = 0; row < 16; ++row) {
        int64_t b = (int64_t)tile * 16 + row;
        if (b >= p.B) break;                                      // rows of no window hold zero gradients
        const int64_t s = tr_start(p, b);
        for (int t = tc * TR_TCHUNK; t < t1; ++t) {
            const float gh = p.S[base + ((int64_t)t * 5 + 1 + g) * step + row * Up + j];
            const float gx = g == 2 ? p.S[base + ((int64_t)t * 5 + 4) * step + row * Up + j] : gh;
            const int c = tr_channel(p, s, t, dir);
            const float gm = gx * (p.masks ? p.masks[(b * 2 + dir) * 5 + c] : 1.0f);
            bh += gh;
            bx += gx;
            for (int k = 0; k < 5; ++k) w[k] += k == c ? gm : 0.0f;
        }
    }
    float *out = p.PW + ((int64_t)chunk * p.ntc + tc) * 7 * G3 + n;
    for (int k = 0; k < 5; ++k) out[k * G3] = w[k];
    out[5 * G3] = bx;
    out[6 * G3] = bh;
}

// every gradient element: the sum of its partials in index order
__global__ void train_reduce_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (!p.grads || e >= p.total) return;
    const int u = p.u, Up = p.Up, G3 = 3 * Up, nchunk = 2 * p.nt;
    float s = 0.0f;
    if (e < p.oU || (e >= p.oB && e < p.oS)) {
        const int k = e < p.oU ? e / (3 * u) : 5 + (e - p.oB) / (3 * u);
        const int col = (e < p.oU ? e : e - p.oB) % (3 * u);
        const int n = (col / u) * Up + col % u;
        const int64_t np = (int64_t)nchunk * p.ntc;
        for (int64_t i = 0; i < np; ++i) s += p.PW[(i * 7 + k) * G3 + n];
    } else if (e < p.oB) {
        const int i = (e - p.oU) / (3 * u), col = (e - p.oU) % (3 * u);
        const int64_t o = (int64_t)i * G3 + (col / u) * Up + col % u;
        for (int c = 0; c < nchunk; ++c) s += p.PU[(int64_t)c * Up * G3 + o];
    } else {
        const int hidx = e - p.oS;
        for (int64_t b = 0; b < p.B; ++b) s += p.PH[b * p.nh + hidx];
    }
    p.grads[e] = s;
}

__global__ void train_loss_kernel(train_table tab)
{
    const train_params &p = tab.job[blockIdx.z];
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.0f;
    for (int64_t b = 0; b < p.B; ++b) s += p.LOSSP[b];
    p.loss[0] = s / ((float)p.B * (float)p.T);
}

int train_layout(train_params &p, int T, int u, int C, int attention, int64_t B)
{
    DGRP_REQUIRE(T >= 1 && T <= 4096, "training: vecsize %d outside 1..4096", T);
    DGRP_REQUIRE(u >= 1 && u <= 256, "training: %d units outside 1..256", u);
    DGRP_REQUIRE(C >= 2 && C <= TR_MAXC, "training: %d classes outside 2..16", C);
    DGRP_REQUIRE(B >= 1 && B <= (1 << 18), "training: batch size %lld outside 1..2^18", (long long)B);
    p.T = T; p.u = u; p.C = C; p.att = attention ? 1 : 0; p.B = B;
    p.Up = (u + 15) / 16 * 16;
    p.F = p.att ? 2 * u : u;
    p.nt = (int)((B + 15) / 16);
    p.ntc = (T + TR_TCHUNK - 1) / TR_TCHUNK;
    p.oK = 0; p.oU = 15 * u; p.oB = p.oU + 3 * u * u; p.oS = p.oB + 6 * u;
    p.oFk = p.oS + (p.att ? u : 0); p.oFb = p.oFk + p.F * C; p.total = p.oFb + C;
    p.nh = p.total - p.oS;
    p.nthr = p.Up <= 64 ? 256 : 512;
    return DGRP_OK;
}

// carve the workspace (base may be null: sizes only); returns the bytes used
int64_t train_carve(train_params &p, void *base)
{
    int64_t off = 0;
    auto take = [&](int64_t floats) {
        float *r = base ? (float *)((char *)base + off) : nullptr;
        off += dgrp_align_up(floats * 4, 256);
        return r;
    };
    const int64_t Up = p.Up, rows = (int64_t)p.nt * p.T;
    p.Upad = take(Up * 3 * Up);
    p.UTpad = take(Up * 3 * Up);
    p.S = take(2 * rows * 5 * 16 * Up);
    p.AVG = take(p.B * p.T * p.u);
    p.DAVG = take(p.B * p.T * p.u);
    p.DL = take(p.B * p.T * p.C);
    p.PH = take(p.B * p.nh);
    p.LOSSP = take(p.B);
    p.PU = take(2 * (int64_t)p.nt * Up * 3 * Up);
    p.PW = take(2 * (int64_t)p.nt * p.ntc * 7 * 3 * Up);
    return off;
}

}   // namespace

DGRP_EXPORT int64_t dgrp_train_param_count(int u, int C, int attention)
{
    train_params p;
    if (train_layout(p, 1, u, C, attention, 1) != DGRP_OK) return 0;
    return p.total;
}

DGRP_EXPORT int64_t dgrp_train_workspace_bytes(int T, int u, int C, int attention, int64_t B)
{
    train_params p;
    if (train_layout(p, T, u, C, attention, B) != DGRP_OK) return 0;
    return train_carve(p, nullptr);
}

namespace {

// checks one job and fills its parameters; launches nothing
int train_prepare(train_params &p, const dgrp_train_job &j)
{
    const int rc = train_layout(p, j.T, j.u, j.C, j.attention, j.B);
    if (rc != DGRP_OK) return rc;
    DGRP_REQUIRE(j.d_params && j.d_idx && j.d_truth && j.d_starts && j.d_loss, "training: NULL parameter, index, truth, start or loss pointer");
    DGRP_REQUIRE(j.n >= j.T, "training: record of %lld bases is shorter than the window (%d)", (long long)j.n, j.T);
    DGRP_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 15) == 0, "training: workspace NULL or not 16-byte aligned");
    if (j.work_bytes < train_carve(p, j.d_work)) {
        dgrp_set_error("training: workspace of %lld bytes, %lld needed", (long long)j.work_bytes, (long long)train_carve(p, nullptr));
        return DGRP_ENOMEM;
    }
    p.n = j.n; p.w = j.d_params; p.idx = j.d_idx; p.truth = j.d_truth; p.starts = j.d_starts; p.masks = j.d_masks;
    p.loss = j.d_loss; p.grads = j.d_grads;
    return DGRP_OK;
}

// the launch chain over the K jobs of `tab`: every extent is the largest any job needs
int train_launch(const train_table &tab, int K, hipStream_t s)
{
    unsigned pack = 0, nt = 0, B = 0, wg = 0, ntc = 0, g3 = 0, red = 0, nthr = 0;
    size_t lds_fwd = 0, lds_bwd = 0, lds_head = 0;
    bool grads = false;
    for (int k = 0; k < K; ++k) {
        const train_params &p = tab.job[k];
        const unsigned Up = p.Up, HS = Up + 4, G3 = 3 * Up;
        pack = std::max(pack, (Up * G3 + 255) / 256);
        nt = std::max(nt, (unsigned)p.nt);
        B = std::max(B, (unsigned)p.B);
        nthr = std::max(nthr, (unsigned)p.nthr);
        lds_fwd = std::max(lds_fwd, 16 * 8 + (size_t)4 * (16 * HS + 16 * G3 + 21 * p.u + 80 + 16));
        lds_head = std::max(lds_head, (size_t)4 * (p.F * p.C + 16 + 3 * p.u + 32 + 2 * p.T + 256 + 256 * (p.C + 2)));
        if (!p.grads) continue;
        grads = true;
        lds_bwd = std::max(lds_bwd, (size_t)4 * (16 * HS + 16 * (G3 + 4)));
        wg = std::max(wg, ((Up / 16) * (G3 / 16) + 3) / 4);
        ntc = std::max(ntc, (unsigned)p.ntc);
        g3 = std::max(g3, G3);
        red = std::max(red, ((unsigned)p.total + 255) / 256);
    }
    static std::once_flag configured;
    static hipError_t cfg_err = hipSuccess;
    std::call_once(configured, [] {
        auto set = [](const void *f) { const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024); if (e != hipSuccess) cfg_err = e; };
        set((const void *)train_forward_kernel);
        set((const void *)train_backward_kernel);
        set((const void *)train_head_kernel);
    });
    DGRP_HIP(cfg_err);
    hipLaunchKernelGGL(train_pack_kernel, dim3(pack, 1, K), dim3(256), 0, s, tab);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_forward_kernel, dim3(nt, 2, K), dim3(nthr), lds_fwd, s, tab);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_head_kernel, dim3(B, 1, K), dim3(256), lds_head, s, tab);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_loss_kernel, dim3(1, 1, K), dim3(64), 0, s, tab);
    DGRP_LAUNCH_CHECK();
    if (!grads) return DGRP_OK;
    hipLaunchKernelGGL(train_backward_kernel, dim3(nt, 2, K), dim3(nthr), lds_bwd, s, tab);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_wgrad_kernel, dim3(wg, 2 * nt, K), dim3(256), 0, s, tab);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_colsum_kernel, dim3(2 * nt, ntc, K), dim3(g3), 0, s, tab);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_reduce_kernel, dim3(red, 1, K), dim3(256), 0, s, tab);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

}   // namespace

DGRP_EXPORT int dgrp_train_step(int T, int u, int C, int attention, const float *d_params, const uint8_t *d_idx,
                                const int8_t *d_truth, int64_t n, const int64_t *d_starts, int64_t B, const float *d_masks,
                                float *d_loss, float *d_grads, void *d_work, int64_t work_bytes, void *stream)
{
    const dgrp_train_job job = {T, u, C, attention, d_params, d_idx, d_truth, n, d_starts, B, d_masks, d_loss, d_grads, d_work, work_bytes};
    train_table tab = {};
    const int rc = train_prepare(tab.job[0], job);
    if (rc != DGRP_OK) return rc;
    return train_launch(tab, 1, (hipStream_t)stream);
}

DGRP_EXPORT int dgrp_train_step_multi(const dgrp_train_job *h_jobs, int K, void *stream)
{
    DGRP_REQUIRE(K >= 1 && K <= DGRP_TRAIN_MAX_JOBS, "training: %d jobs outside 1..%d", K, DGRP_TRAIN_MAX_JOBS);
    DGRP_REQUIRE(h_jobs, "training: NULL job list");
    train_table tab = {};
    int64_t used[DGRP_TRAIN_MAX_JOBS];
    for (int k = 0; k < K; ++k) {
        const int rc = train_prepare(tab.job[k], h_jobs[k]);
        if (rc != DGRP_OK) {
            char msg[512];
            snprintf(msg, sizeof msg, "%s", dgrp_last_error());
            dgrp_set_error("job %d: %s", k, msg);
            return rc;
        }
        used[k] = train_carve(tab.job[k], h_jobs[k].d_work);
        for (int i = 0; i < k; ++i) {
            const char *a = (const char *)h_jobs[i].d_work, *b = (const char *)h_jobs[k].d_work;
            DGRP_REQUIRE(a + used[i] <= b || b + used[k] <= a, "job %d: training: workspace overlaps the workspace of job %d", k, i);
        }
    }
    return train_launch(tab, K, (hipStream_t)stream);
}
