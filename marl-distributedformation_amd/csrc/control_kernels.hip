// gfx950 kernels of the baseline formation controller (reference: /root/reference/simulate.py
// :256-319 control(), the potential-field controller the paper's RL policy is compared with) and
// of the simulator's velocity step (simulate.py:70 FormationSimulator.step(input_velocity)),
// fused into T-step rollouts.
//
// Mapping and numerics are those of fenv_kernels.hip: one lane owns one agent for the whole
// launch, a wavefront holds 64/N whole formations for N <= 64 (k_control_rollout_wave), one
// workgroup one formation for 64 < N <= 1024 (k_control_rollout_block); contraction is off,
// division and sqrt are the correctly rounded IEEE ops, and every expression keeps the
// reference's operation order (comments cite the line), so the velocities are the reference's
// bit for bit.  Per step: one exchange round for the previous, next and opposite agents'
// positions, the controller, then the env step and the observation of env_device.h.
// Formations above 1,024 agents are not covered (fenv_api.cpp rejects them).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "env_device.h"

namespace fenvk {

// torch.clip(v, -1, 1) incl. NaN propagation (simulate.py:293, :317)
__device__ __forceinline__ float clip1(float v) {
    return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}

// One spring term of f_formation (simulate.py:270-275 / :282-284, :290-292) of the agent at
// (px, py) towards the agent at (qx, qy) with rest length `des`.
__device__ __forceinline__ void ctl_term(float px, float py, float qx, float qy, float des,
                                         float &tx, float &ty) {
    const float d = norm2(px - qx, py - qy);  // :270 norm(agents - shift)
    const float dx = (qx - px) / d;           // :271-272 (shift - agents) / dist
    const float dy = (qy - py) / d;
    const float m = 0.02f * (d - des);        // :290 the scalar first
    tx = m * dx;
    ty = m * dy;
}

// control() (simulate.py:256-319) for this lane's agent: the velocity it hands to env.step.
// dd = pi * desired_radius / num_agents (:286, desired_radius = 40 at :259 -- not the reward's
// 60), rounded to fp32 where it meets the fp32 tensor.  Coincident agents divide 0 by 0 as the
// reference does.
template <class X>
__device__ __forceinline__ void control_velocity(const X &x, const Agent &s, float dd, float &vx,
                                                 float &vy) {
    float ppx, pnx, pox, ppy, pny, poy;
    x.q_pno(s.px, s.py, ppx, pnx, pox, ppy, pny, poy);
    float ax, ay, bx, by, ox, oy;
    ctl_term(s.px, s.py, pnx, pny, dd, ax, ay);     // :262-264 agents_shiftA = the next agent
    ctl_term(s.px, s.py, ppx, ppy, dd, bx, by);     // :265-267 agents_shiftB = the previous one
    ctl_term(s.px, s.py, pox, poy, 80.0f, ox, oy);  // :278-284, 2 * desired_radius
    const float ffx = clip1((ax + bx) + ox);        // :290-293
    const float ffy = clip1((ay + by) + oy);
    const float gdx = s.px - s.gx;                  // :311
    const float gdy = s.py - s.gy;
    const float d = norm2(gdx, gdy);                // :312
    const float m = -(0.01f * (d - 40.0f));         // :315-316
    const float fgx = clip1(m * (gdx / d));         // :313, :316-317
    const float fgy = clip1(m * (gdy / d));
    // :319 f_formation + f_obstacle + f_goal; f_obstacle is zeros (no obstacles, :16): the
    // + 0.0f turns a -0.0 of f_formation into +0.0
    vx = (ffx + 0.0f) + fgx;
    vy = (ffy + 0.0f) + fgy;
}

// Velocity source of a rollout: computed by the controller from the state in registers, or read
// from HBM (fenv_rollout_velocity).
constexpr int kVelControl = 0, kVelHBM = 1;

template <int D, int MODE, int VS, class X>
__device__ __forceinline__ void control_rollout_body(const Consts &c, const DevState &st,
                                                     const DevPending &p, const X &x, bool active,
                                                     int64_t f, int64_t a, int i, float *stage,
                                                     int lane, int M, int64_t a_first, int32_t T,
                                                     float dd, const float2 *__restrict__ vel_in,
                                                     float2 *__restrict__ vel_out,
                                                     float *__restrict__ obs,
                                                     float *__restrict__ rew,
                                                     uint8_t *__restrict__ done, float &rsum,
                                                     float &dsum) {
    const int64_t A = c.F * (int64_t)c.N;
    Agent s{0.f, 0.f, 0.f, 0.f, 0, 0u};
    if (active) {
        s.px = st.px[a];
        s.py = st.py[a];
        s.gx = st.gx[f];
        s.gy = st.gy[f];
        s.t = st.t[f];
        s.ep = st.ep[f];
    }
    bool any_reset = false;
    for (int32_t k = 0; k < T; ++k) {
        const int64_t row = (int64_t)k * A + a;
        float vx = 0.f, vy = 0.f;
        if (VS == kVelControl) {
            control_velocity(x, s, dd, vx, vy);
            if (!active) {  // a lane that owns no agent: zero velocity, nothing stored
                vx = 0.f;
                vy = 0.f;
            } else if (vel_out) {
                vel_out[row] = make_float2(vx, vy);
            }
        } else if (active) {
            const float2 v = vel_in[row];
            vx = v.x;
            vy = v.y;
        }
        float rw;
        bool dn, rs;
        env_step_v<MODE, X>(c, p, x, f, a, i, active, vx, vy, s, rw, dn, rs);
        any_reset |= rs;
        if (obs) {
            float o[8];
            env_obs<D>(x, s, o);
            store_obs_rows<D>(stage, o, lane, M, obs + ((int64_t)k * A + a_first) * D);
        }
        if (active) {
            if (rew) rew[row] = rw;
            if (done) done[row] = (uint8_t)dn;
            rsum += rw;
            dsum += dn ? 1.0f : 0.0f;
        }
    }
    if (active) {
        st.px[a] = s.px;
        st.py[a] = s.py;
        if (i == 0) {
            st.t[f] = s.t;
            if (any_reset) {
                st.gx[f] = s.gx;
                st.gy[f] = s.gy;
                st.ep[f] = s.ep;
            }
        }
    }
}

// Lane mapping of the wave path (as k_rollout_wave): lanes fi*N .. fi*N+N-1 of a wavefront own
// formation wave * fpw + fi; the opposite agent's lane is lane + N/2 for i < N/2, else lane - N/2.
struct WaveMap {
    int lane, i, M;
    int64_t f, a, a_first;
    bool active;
    WaveX x;
    __device__ __forceinline__ WaveMap(const Consts &c) {
        lane = threadIdx.x & 63;
        const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        const int N = c.N, h = N >> 1;
        const int fi = lane / N;
        i = lane - fi * N;
        f = wave * c.fpw + fi;
        active = fi < c.fpw && f < c.F;
        a = f * N + i;
        x = WaveX{i == 0 ? lane + N - 1 : lane - 1, i == N - 1 ? lane - N + 1 : lane + 1,
                  i < h ? lane + h : lane - h};
        const int64_t f_first = wave * c.fpw;
        const int64_t f_left = c.F - f_first;
        M = (int)((f_left <= 0 ? 0 : (f_left < c.fpw ? f_left : c.fpw)) * N);
        a_first = f_first * N;
    }
};

// Ring indices of the block path: a thread past N exchanges with itself.
__device__ __forceinline__ BlockX block_x(float *lds, int i, int N) {
    const bool active = i < N;
    const int h = N >> 1;
    return BlockX{lds, i, active ? (i == 0 ? N - 1 : i - 1) : i,
                  active ? (i == N - 1 ? 0 : i + 1) : i, active ? (i < h ? i + h : i - h) : i};
}

template <int D, int MODE, int VS>
__global__ __launch_bounds__(256) void k_control_rollout_wave(
    Consts c, DevState st, DevPending p, int32_t T, float dd, const float2 *__restrict__ vel_in,
    float2 *__restrict__ vel_out, float *__restrict__ obs, float *__restrict__ rew,
    uint8_t *__restrict__ done, float2 *__restrict__ partial, bool accum) {
    // No early exit for waves past the last formation (the workgroup reduction has a barrier).
    __shared__ __attribute__((aligned(16))) float stage[4][64 * 8];
    __shared__ float2 red[4];
    const int w = threadIdx.x >> 6;
    const WaveMap m(c);
    float rsum = 0.f, dsum = 0.f;
    if (m.M > 0)
        control_rollout_body<D, MODE, VS, WaveX>(c, st, p, m.x, m.active, m.f, m.a, m.i, stage[w],
                                                 m.lane, m.M, m.a_first, T, dd, vel_in, vel_out,
                                                 obs, rew, done, rsum, dsum);
    if (partial) {  // k_rollout_wave's records: one {sum reward, sum done} per workgroup
        rsum = wave_sum(rsum);
        dsum = wave_sum(dsum);
        if (m.lane == 0) red[w] = make_float2(rsum, dsum);
        __syncthreads();
        if (threadIdx.x == 0) {
            float2 v = red[0];
            for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
                v = make_float2(v.x + red[k].x, v.y + red[k].y);
            if (accum) v = make_float2(partial[blockIdx.x].x + v.x, partial[blockIdx.x].y + v.y);
            partial[blockIdx.x] = v;
        }
    }
}

template <int D, int MODE, int VS>
__global__ __launch_bounds__(1024) void k_control_rollout_block(
    Consts c, DevState st, DevPending p, int32_t T, float dd, const float2 *__restrict__ vel_in,
    float2 *__restrict__ vel_out, float *__restrict__ obs, float *__restrict__ rew,
    uint8_t *__restrict__ done, float2 *__restrict__ partial, bool accum) {
    __shared__ float lds[7 * kMaxN];
    __shared__ float red[2][kMaxN / 64];
    __shared__ __attribute__((aligned(16))) float stage[kMaxN / 64][64 * 8];
    const int N = c.N;
    const int i = threadIdx.x;
    const int64_t f = blockIdx.x;
    const bool active = i < N;
    const int64_t a = f * N + i;
    const BlockX x = block_x(lds, i, N);
    const int w = i >> 6;
    const int M = N - 64 * w < 64 ? (N - 64 * w > 0 ? N - 64 * w : 0) : 64;
    float rsum = 0.f, dsum = 0.f;
    control_rollout_body<D, MODE, VS, BlockX>(c, st, p, x, active, f, a, i, stage[w], i & 63, M,
                                              f * N + 64 * w, T, dd, vel_in, vel_out, obs, rew,
                                              done, rsum, dsum);
    if (partial) {  // k_rollout_block's records: one per formation
        rsum = wave_sum(rsum);
        dsum = wave_sum(dsum);
        const int nw = blockDim.x >> 6;
        if ((i & 63) == 0) {
            red[0][w] = rsum;
            red[1][w] = dsum;
        }
        __syncthreads();
        if (i == 0) {
            float r = 0.f, d = 0.f;
            for (int k = 0; k < nw; ++k) {
                r += red[0][k];
                d += red[1][k];
            }
            if (accum) {
                r = partial[f].x + r;
                d = partial[f].y + d;
            }
            partial[f] = make_float2(r, d);
        }
    }
}

// ---------------------------------------------------------------- velocities only
// control() without the step: the state is read, not written.
__global__ __launch_bounds__(256) void k_control_wave(Consts c, DevState st, float dd,
                                                      float2 *__restrict__ vel) {
    const WaveMap m(c);
    if (m.M == 0) return;  // wave-uniform: no lane of the wave owns an agent
    Agent s{0.f, 0.f, 0.f, 0.f, 0, 0u};
    if (m.active) {
        s.px = st.px[m.a];
        s.py = st.py[m.a];
        s.gx = st.gx[m.f];
        s.gy = st.gy[m.f];
    }
    float vx, vy;
    control_velocity(m.x, s, dd, vx, vy);
    if (m.active) vel[m.a] = make_float2(vx, vy);
}

__global__ __launch_bounds__(1024) void k_control_block(Consts c, DevState st, float dd,
                                                        float2 *__restrict__ vel) {
    __shared__ float lds[7 * kMaxN];
    const int N = c.N;
    const int i = threadIdx.x;
    const int64_t f = blockIdx.x;
    const bool active = i < N;
    const int64_t a = f * N + i;
    const BlockX x = block_x(lds, i, N);
    Agent s{0.f, 0.f, 0.f, 0.f, 0, 0u};
    if (active) {
        s.px = st.px[a];
        s.py = st.py[a];
        s.gx = st.gx[f];
        s.gy = st.gy[f];
    }
    float vx, vy;
    control_velocity(x, s, dd, vx, vy);
    if (active) vel[a] = make_float2(vx, vy);
}

// ---------------------------------------------------------------- launchers
static inline unsigned block_threads(int32_t N) { return (unsigned)((N + 63) / 64 * 64); }

template <int D, int MODE, int VS>
static hipError_t control_rollout_dmv(const Consts &c, const DevState &s, const DevPending &p,
                                      int32_t T, float dd, const float *vel_in, float *vel_out,
                                      float *obs, float *rew, uint8_t *done, float *partial,
                                      bool accum, hipStream_t st) {
    const float2 *vi = reinterpret_cast<const float2 *>(vel_in);
    float2 *vo = reinterpret_cast<float2 *>(vel_out);
    float2 *p2 = reinterpret_cast<float2 *>(partial);
    if (wave_path(c.N))
        hipLaunchKernelGGL((k_control_rollout_wave<D, MODE, VS>), dim3((unsigned)group_count(c)),
                           dim3(256), 0, st, c, s, p, T, dd, vi, vo, obs, rew, done, p2, accum);
    else
        hipLaunchKernelGGL((k_control_rollout_block<D, MODE, VS>), dim3((unsigned)c.F),
                           dim3(block_threads(c.N)), 0, st, c, s, p, T, dd, vi, vo, obs, rew, done,
                           p2, accum);
    return hipGetLastError();
}

template <int D, int MODE>
static hipError_t control_rollout_dm(const Consts &c, const DevState &s, const DevPending &p,
                                     int32_t T, float dd, bool computed, const float *vel_in,
                                     float *vel_out, float *obs, float *rew, uint8_t *done,
                                     float *partial, bool accum, hipStream_t st) {
    return computed ? control_rollout_dmv<D, MODE, kVelControl>(c, s, p, T, dd, nullptr, vel_out,
                                                                obs, rew, done, partial, accum, st)
                    : control_rollout_dmv<D, MODE, kVelHBM>(c, s, p, T, dd, vel_in, nullptr, obs,
                                                            rew, done, partial, accum, st);
}

hipError_t launch_control_rollout(const Consts &c, const DevState &s, const DevPending &p,
                                  int32_t T, int32_t D, float dd, bool computed,
                                  const float *vel_in, float *vel_out, float *obs, float *rew,
                                  uint8_t *done, float *partial, bool accum, hipStream_t st) {
    if (large_path(c.N)) return hipErrorInvalidValue;
    const bool mt = c.reset_mode == FENV_RESET_MT19937;
    if (D == 8)
        return mt ? control_rollout_dm<8, FENV_RESET_MT19937>(c, s, p, T, dd, computed, vel_in,
                                                              vel_out, obs, rew, done, partial,
                                                              accum, st)
                  : control_rollout_dm<8, FENV_RESET_PHILOX>(c, s, p, T, dd, computed, vel_in,
                                                             vel_out, obs, rew, done, partial,
                                                             accum, st);
    return mt ? control_rollout_dm<6, FENV_RESET_MT19937>(c, s, p, T, dd, computed, vel_in,
                                                          vel_out, obs, rew, done, partial, accum,
                                                          st)
              : control_rollout_dm<6, FENV_RESET_PHILOX>(c, s, p, T, dd, computed, vel_in,
                                                         vel_out, obs, rew, done, partial, accum,
                                                         st);
}

hipError_t launch_control(const Consts &c, const DevState &s, float dd, float *vel,
                          hipStream_t st) {
    if (large_path(c.N)) return hipErrorInvalidValue;
    float2 *v2 = reinterpret_cast<float2 *>(vel);
    if (wave_path(c.N))
        hipLaunchKernelGGL(k_control_wave, dim3((unsigned)group_count(c)), dim3(256), 0, st, c, s,
                           dd, v2);
    else
        hipLaunchKernelGGL(k_control_block, dim3((unsigned)c.F), dim3(block_threads(c.N)), 0, st,
                           c, s, dd, v2);
    return hipGetLastError();
}

}  // namespace fenvk
