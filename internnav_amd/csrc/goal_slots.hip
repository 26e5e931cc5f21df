// Goal rows of the NavDPNet condition for a batch of envs whose goals are of different kinds, in one launch (gfx950).
//
// NavDPNet.predict_noise (navdp_policy.py:159-170) writes ONE goal embedding e [D] into condition slots 1, 2 and 3 of an env, whatever
// produced it: zeros (no goal), point_encoder = Linear(3, D) of the point goal, or ImageGoalBackbone / PixelGoalBackbone.forward
// (navdp_backbone.py:340-346, 391-397) = project_layer(mean over the 256 final-LayerNorm patch tokens of a ViT-S). The towers run over
// compact sub-batches (only the envs of their kind); this kernel finishes every env: one workgroup per env reads the env's kind and its row
// in the compact input of that kind, forms e in fp32 and writes e + cond_pos_embed[slot] to the slots (and, optionally, e itself).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kMaxWidth = 1024;   // D and E bound (LDS rows below); NavDPNet uses 384 for both

struct GoalSlotsArgs {
    void* Y;
    const float* P;
    float* embed;
    const int32_t* kind;
    const int32_t* row;
    const float* point;
    const float* point_w;
    const float* point_b;
    const float* tok[2];    // image, pixel tower tokens f32 [n * ntok, E]
    const float* w[2];      // project_layer weights f32 [D, E]
    const float* b[2];      // project_layer biases f32 [D]
    int32_t n[3];           // rows of the point / image / pixel inputs
    int32_t ldy, y_dtype, L, slot0, nslots, D, ntok, E;
};

template <bool OUT_F32>
__global__ __launch_bounds__(256) void goal_slots_kernel(GoalSlotsArgs p) {
    __shared__ float part[kMaxWidth];   // per-phase partial sums of the token mean
    __shared__ float mean[kMaxWidth];
    __shared__ float emb[kMaxWidth];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k = p.kind[b], r = p.row[b];          // uniform over the workgroup: the __syncthreads below sit in uniform branches
    const bool bad = k < 0 || k > 3 || (k > 0 && (r < 0 || r >= p.n[k - 1]));
    if (bad) {                                      // the host validates the plan; a bad entry poisons its rows instead of reading out of bounds
        for (int d = tid; d < p.D; d += 256) emb[d] = __builtin_nanf("");
    } else if (k == 0) {
        for (int d = tid; d < p.D; d += 256) emb[d] = 0.f;
    } else if (k == 1) {
        const float* x = p.point + (size_t)r * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        for (int d = tid; d < p.D; d += 256) {      // the arithmetic of embed3, so a point env gets the bits of the point-goal call
            float a = ina_dot3(p.point_w[d * 3], p.point_w[d * 3 + 1], p.point_w[d * 3 + 2], x0, x1, x2);
            a += p.point_b[d];
            emb[d] = a;
        }
    } else {
        const int t = k - 2;
        // fp32 mean over the env's ntok tokens: thread = (phase, group of 4 channels); phases stride the tokens, 16-byte loads
        const int E4 = p.E >> 2, phases = 256 / E4;
        const int g = tid % E4, ph = tid / E4;
        if (ph < phases) {
            const float* src = p.tok[t] + (size_t)r * p.ntok * p.E + g * 4;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            int i = ph;
            for (; i + 3 * phases < p.ntok; i += 4 * phases) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + (size_t)i * p.E);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + (size_t)(i + phases) * p.E);
                const f32x4 v2 = *reinterpret_cast<const f32x4*>(src + (size_t)(i + 2 * phases) * p.E);
                const f32x4 v3 = *reinterpret_cast<const f32x4*>(src + (size_t)(i + 3 * phases) * p.E);
                acc += v0;
                acc += v1;
                acc += v2;
                acc += v3;
            }
            for (; i < p.ntok; i += phases) acc += *reinterpret_cast<const f32x4*>(src + (size_t)i * p.E);
            *reinterpret_cast<f32x4*>(&part[ph * p.E + g * 4]) = acc;
        }
        __syncthreads();
        const float inv = 1.f / (float)p.ntok;
        for (int c = tid; c < p.E; c += 256) {
            float s = 0.f;
            for (int q = 0; q < phases; ++q) s += part[q * p.E + c];
            mean[c] = s * inv;
        }
        __syncthreads();
        // project_layer: each wave owns outputs d = wave, wave + 4, ...; its lanes read one weight row coalesced and reduce by shuffles
        const int wave = tid >> 6, lane = tid & 63;
        const float* W = p.w[t];
        for (int d = wave; d < p.D; d += 4) {
            const float* wr = W + (size_t)d * p.E;
            float a = 0.f;
            for (int c = lane; c < p.E; c += 64) a += wr[c] * mean[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
            if (lane == 0) emb[d] = a + p.b[t][d];
        }
    }
    __syncthreads();
    for (int i = tid; i < p.nslots * p.D; i += 256) {
        const int j = i / p.D, d = i - j * p.D;
        float v = emb[d];
        if (p.P) v += p.P[(size_t)(p.slot0 + j) * p.D + d];
        const size_t o = ((size_t)b * p.L + p.slot0 + j) * p.ldy + d;
        if (OUT_F32) reinterpret_cast<float*>(p.Y)[o] = v;
        else reinterpret_cast<bf16*>(p.Y)[o] = (bf16)v;
    }
    if (p.embed)
        for (int d = tid; d < p.D; d += 256) p.embed[(size_t)b * p.D + d] = emb[d];
}

}  // namespace

int ina_launch_goal_slots(void* Y, int ldy, int y_dtype, int L, int slot0, int nslots, const float* P, int B, int D, const int32_t* kind,
                          const int32_t* row, float* embed, const float* point, int n_point, const float* point_w, const float* point_b,
                          const float* image_tok, int n_image, const float* image_w, const float* image_b, const float* pixel_tok,
                          int n_pixel, const float* pixel_w, const float* pixel_b, int ntok, int E, hipStream_t stream) {
    INA_REQUIRE(Y && kind && row && B > 0 && D > 0 && D <= kMaxWidth && ldy >= D && L > 0 && slot0 >= 0 && nslots > 0 && slot0 + nslots <= L,
                "goal_slots: bad arguments B=%d D=%d ldy=%d L=%d slots %d..%d", B, D, ldy, L, slot0, slot0 + nslots - 1);
    INA_REQUIRE(y_dtype == INA_DT_F32 || y_dtype == INA_DT_BF16, "goal_slots: y_dtype %d", y_dtype);
    INA_REQUIRE(n_point >= 0 && n_image >= 0 && n_pixel >= 0, "goal_slots: negative row counts");
    INA_REQUIRE(n_point == 0 || (point && point_w && point_b), "goal_slots: point goals need point, point_w and point_b");
    auto al16 = [](const void* q) { return ((uintptr_t)q % 16) == 0; };
    const bool towers = n_image > 0 || n_pixel > 0;
    if (towers) {
        INA_REQUIRE(ntok > 0 && E > 0 && E % 4 == 0 && E <= kMaxWidth, "goal_slots: tower tokens ntok=%d E=%d (E a multiple of 4, <= %d)", ntok, E,
                    kMaxWidth);
    }
    INA_REQUIRE(n_image == 0 || (image_tok && image_w && image_b && al16(image_tok)), "goal_slots: image goals need 16-byte aligned image_tok, image_w, image_b");
    INA_REQUIRE(n_pixel == 0 || (pixel_tok && pixel_w && pixel_b && al16(pixel_tok)), "goal_slots: pixel goals need 16-byte aligned pixel_tok, pixel_w, pixel_b");
    GoalSlotsArgs p{};
    p.Y = Y, p.P = P, p.embed = embed, p.kind = kind, p.row = row;
    p.point = point, p.point_w = point_w, p.point_b = point_b;
    p.tok[0] = image_tok, p.w[0] = image_w, p.b[0] = image_b;
    p.tok[1] = pixel_tok, p.w[1] = pixel_w, p.b[1] = pixel_b;
    p.n[0] = n_point, p.n[1] = n_image, p.n[2] = n_pixel;
    p.ldy = ldy, p.y_dtype = y_dtype, p.L = L, p.slot0 = slot0, p.nslots = nslots, p.D = D, p.ntok = towers ? ntok : 1, p.E = towers ? E : 4;
    const double tok_bytes = 4.0 * (double)(n_image + n_pixel) * ntok * E;
    InaProfScope prof(INA_PROF_ELEMENTWISE, 2.0 * (n_image + n_pixel) * ((double)ntok * E + (double)D * E), tok_bytes +
                      (double)B * nslots * D * (y_dtype == INA_DT_F32 ? 4.0 : 2.0), stream);
    if (y_dtype == INA_DT_F32) hipLaunchKernelGGL(goal_slots_kernel<true>, dim3(B), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(goal_slots_kernel<false>, dim3(B), dim3(256), 0, stream, p);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
