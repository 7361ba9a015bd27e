// rr_render.hpp -- RGB frames of many arenas in one launch, straight from the HBM records (include/roborugby_amd.h: rr_render holds the
// specification of the picture; this file follows it line by line).
//
// One instantiation for every configuration: the record is described by a small runtime struct (RenderLayout, filled from RecLayout<C> /
// Arena<C> where the handle's configuration is known), the shading never sees a Cfg.  A block of 256 threads shades 1,024 consecutive
// pixels of ONE frame (blockIdx.y): its first NR + NB threads turn the arena's entities into a draw list in LDS -- centre, cos / sin of the
// robot's angle, the packed fill colour, all fp32; sin / cos once per robot and block --, one barrier, then every thread shades 4
// horizontally adjacent pixels with uniform loops over that list (LDS broadcast reads) and stores their 12 bytes as three dwords:
// 768 contiguous bytes per wavefront.  Read-only on the records, no atomics; every byte of the frames is written, nothing beyond them.
//
// The draw-list builder, the shading core and the byte packing are RR_HD: the same source compiles with g++ (tests/emu/rr_render_emu.cpp).
#pragma once
#include "rr_sim.hpp"

namespace rr {

constexpr int RENDER_MAX = 16;     // robots resp. balls per arena a draw list holds (the configurations stop at 8 and 11)
constexpr int RENDER_THREADS = 256, RENDER_QUAD = 4; // threads per block; pixels per thread

// packed colour: r | g << 8 | b << 16 -- the order of the bytes in memory
constexpr uint32_t render_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }
constexpr uint32_t RENDER_BACKGROUND = render_rgb(255, 255, 255), RENDER_GOAL_GRUMPY = render_rgb(242, 53, 87),
                   RENDER_GOAL_HAPPY = render_rgb(43, 146, 228), RENDER_BLACK = render_rgb(0, 0, 0), RENDER_FRONT = render_rgb(255, 255, 0),
                   RENDER_TEAM_HAPPY = render_rgb(40, 90, 200), RENDER_TEAM_GRUMPY = render_rgb(200, 60, 60),
                   RENDER_BALL_POS = render_rgb(80, 220, 100), RENDER_BALL_NEG = render_rgb(60, 16, 83);
constexpr uint32_t RENDER_OUTSIDE = render_rgb(96, 96, 96); // egocentric frames only: beyond the walls

// where the five fields a picture needs sit in an arena's record (indices into its stored reals), and what the record is made of
struct RenderLayout {
    int32_t rcx, rcy, rrot, bcx, bcy;
    int32_t stride;            // stored reals per record
    int32_t nr, nrh, nb, nbp;
    int32_t f64;               // the stored reals are doubles (else floats)
};
// the frame: arena size, arena units per sample (computed once on the host), pixels, samples per axis and pixel
struct RenderView {
    float W, H, fx, fy;
    int32_t width, height, S;
};
struct DrawList {
    float rx[RENDER_MAX], ry[RENDER_MAX], rc[RENDER_MAX], rs[RENDER_MAX];
    float bx[RENDER_MAX], by[RENDER_MAX];
    uint32_t rcol[RENDER_MAX], bcol[RENDER_MAX];
};

RR_HD float render_load(const void *rec, int f64, int word) {
    return f64 ? (float)static_cast<const double *>(rec)[word] : static_cast<const float *>(rec)[word];
}
RR_HD bool render_finite(float x) { return x - x == 0.0f; }

// entry t of the draw list (t < nr: robot t; t < nr + nb: ball t - nr) from the arena's record.  An entity with a non-finite pose gets a
// NaN centre: no sample is inside it.
RR_HD void render_build(const RenderLayout &L, const void *rec, int t, DrawList &dl) {
    if (t < L.nr) {
        float x = render_load(rec, L.f64, L.rcx + t), y = render_load(rec, L.f64, L.rcy + t);
        const float rot = render_load(rec, L.f64, L.rrot + t);
        float th = (360.0f - rot) * 0.017453292519943295f; // radians(360 - rot)
        if (!(render_finite(x) && render_finite(y) && render_finite(rot))) { x = NAN; y = NAN; th = 0.0f; }
        dl.rx[t] = x;
        dl.ry[t] = y;
        dl.rc[t] = cosf(th);
        dl.rs[t] = sinf(th);
        dl.rcol[t] = t < L.nrh ? RENDER_TEAM_HAPPY : RENDER_TEAM_GRUMPY;
    } else if (t < L.nr + L.nb) {
        const int b = t - L.nr;
        float x = render_load(rec, L.f64, L.bcx + b), y = render_load(rec, L.f64, L.bcy + b);
        if (!(render_finite(x) && render_finite(y))) { x = NAN; y = NAN; }
        dl.bx[b] = x;
        dl.by[b] = y;
        dl.bcol[b] = b < L.nbp ? RENDER_BALL_POS : RENDER_BALL_NEG;
    }
}

// colour of the sample point (x, y): the topmost layer that contains it -- background, goals, robots 0 .. nr-1, balls 0 .. nb-1, a later
// one over an earlier one; closed boundaries
RR_HD uint32_t render_sample(const DrawList &dl, int nr, int nb, float W, float H, float x, float y) {
    uint32_t col = RENDER_BACKGROUND;
    if (x + y <= 240.0f) col = RENDER_GOAL_GRUMPY;
    if ((W - x) + (H - y) <= 240.0f) col = RENDER_GOAL_HAPPY;
    for (int r = 0; r < nr; r++) {
        const float dx = x - dl.rx[r], dy = y - dl.ry[r], c = dl.rc[r], s = dl.rs[r];
        const float u = dx * c + dy * s, v = dy * c - dx * s; // the inverse of render.robot_corners
        const float au = fabsf(u), av = fabsf(v);
        if (au <= 10.0f && av <= 20.0f) col = (au > 9.0f || av > 19.0f) ? RENDER_BLACK : (u > 7.0f ? RENDER_FRONT : dl.rcol[r]);
    }
    for (int b = 0; b < nb; b++) {
        const float dx = x - dl.bx[b], dy = y - dl.by[b];
        const float d2 = dx * dx + dy * dy;
        if (d2 <= 49.0f) col = d2 > 36.0f ? RENDER_BLACK : dl.bcol[b];
    }
    return col;
}

// pixel (i, j): the rounded mean of its S x S samples, channel by channel (S = 1: the sample itself)
RR_HD uint32_t render_pixel(const DrawList &dl, int nr, int nb, const RenderView &V, int i, int j) {
    const int S = V.S;
    uint32_t sr = 0, sg = 0, sb = 0;
    for (int b = 0; b < S; b++) {
        const float y = ((float)(j * S + b) + 0.5f) * V.fy;
        for (int a = 0; a < S; a++) {
            const float x = ((float)(i * S + a) + 0.5f) * V.fx;
            const uint32_t c = render_sample(dl, nr, nb, V.W, V.H, x, y);
            sr += c & 255u; sg += (c >> 8) & 255u; sb += c >> 16;
        }
    }
    const uint32_t k = (uint32_t)(S * S), h = k / 2;
    return render_rgb((sr + h) / k, (sg + h) / k, (sb + h) / k);
}

// the three dwords of quad q of a frame (pixels 4q .. 4q+3 in row-major order: width % 4 == 0, so a quad never wraps a row);
// valid = false: the frame of an arena index outside 0 .. N-1, all zero
RR_HD void render_quad(const DrawList &dl, int nr, int nb, const RenderView &V, bool valid, size_t q, uint32_t &w0, uint32_t &w1, uint32_t &w2) {
    w0 = 0; w1 = 0; w2 = 0;
    if (!valid) return;
    const int qpr = V.width / RENDER_QUAD; // quads per row
    const int j = (int)(q / (size_t)qpr), i0 = (int)(q % (size_t)qpr) * RENDER_QUAD;
    const uint32_t p0 = render_pixel(dl, nr, nb, V, i0, j), p1 = render_pixel(dl, nr, nb, V, i0 + 1, j),
                   p2 = render_pixel(dl, nr, nb, V, i0 + 2, j), p3 = render_pixel(dl, nr, nb, V, i0 + 3, j);
    w0 = p0 | (p1 << 24);          // r0 g0 b0 r1
    w1 = (p1 >> 8) | (p2 << 16);   // g1 b1 r2 g2
    w2 = (p2 >> 16) | (p3 << 8);   // b2 r3 g3 b3
}

// the arena a frame shows: arenas[frame], or the frame's own index without a list; false: outside 0 .. n-1 (never used as an index)
RR_HD bool render_arena_of(const int32_t *arenas, size_t frame, int n, size_t &arena) {
    const int64_t a = arenas ? (int64_t)arenas[frame] : (int64_t)frame;
    arena = (size_t)(a < 0 ? 0 : a);
    return a >= 0 && a < (int64_t)n;
}
RR_HD const void *render_record(const RenderLayout &L, const void *recs, size_t arena) {
    return static_cast<const char *>(recs) + arena * (size_t)L.stride * (L.f64 ? 8 : 4);
}

// ---- Egocentric frames (include/roborugby_amd.h: rr_render_ego holds the specification).  The same draw list, layers and box filter seen
// from ONE robot: centred on it (or `ahead` in front of it), its front up, optionally coloured from its own side, and one layer on top --
// OUTSIDE beyond the walls.  What is per frame is decided once per block, not per sample: the camera is the viewer's draw-list entry, the
// palette swap goes into the draw list's colours and into two goal-colour values.
constexpr int32_t RENDER_EGO_RELATIVE = 1, RENDER_EGO_PLANAR = 2; // RR_EGO_RELATIVE, RR_EGO_PLANAR

// the frame: arena size, arena units per sample, half the extent across and down, the shift forward (all computed once on the host)
struct EgoView {
    float W, H, f, hx, hy, ahead;
    int32_t width, height, S, flags;
};
struct EgoCamera {
    float cx, cy, c, s;
    uint32_t goal_grumpy, goal_happy; // the colours of the two goals as the viewer sees them
};

inline EgoView render_ego_view(double W, double H, int width, int height, int S, double span, double ahead, int flags) {
    return { (float)W, (float)H, (float)(span / (double)(width * S)), (float)(span * 0.5), (float)(span * 0.5 * height / width), (float)ahead,
             width, height, S, flags };
}

// the robot a frame is seen from: robots[frame], or robot 0 without a list; false: outside 0 .. nr-1 (never used as an index)
RR_HD bool render_viewer_of(const int32_t *robots, size_t frame, int nr, int &viewer) {
    const int32_t r = robots ? robots[frame] : 0;
    viewer = r < 0 ? 0 : r;
    return r >= 0 && r < nr;
}
// the viewer's palette is swapped pairwise -- team, ball and goal colours -- when it asks for its own side's colours and is grumpy
RR_HD bool render_ego_swap(const RenderLayout &L, int flags, int viewer) { return (flags & RENDER_EGO_RELATIVE) && viewer >= L.nrh; }

// entry t of the draw list as the viewer sees it
RR_HD void render_build_ego(const RenderLayout &L, const void *rec, int t, bool swap, DrawList &dl) {
    render_build(L, rec, t, dl);
    if (!swap) return;
    if (t < L.nr) dl.rcol[t] = t < L.nrh ? RENDER_TEAM_GRUMPY : RENDER_TEAM_HAPPY;
    else if (t < L.nr + L.nb) dl.bcol[t - L.nr] = t - L.nr < L.nbp ? RENDER_BALL_NEG : RENDER_BALL_POS;
}
// the camera from the finished draw list; false: the viewer's pose is non-finite (render_build gave it a NaN centre)
RR_HD bool render_camera(const DrawList &dl, int viewer, bool swap, EgoCamera &cam) {
    cam.cx = dl.rx[viewer]; cam.cy = dl.ry[viewer]; cam.c = dl.rc[viewer]; cam.s = dl.rs[viewer];
    cam.goal_grumpy = swap ? RENDER_GOAL_HAPPY : RENDER_GOAL_GRUMPY;
    cam.goal_happy = swap ? RENDER_GOAL_GRUMPY : RENDER_GOAL_HAPPY;
    return render_finite(cam.cx) && render_finite(cam.cy);
}

// render_sample's layers with the viewer's goal colours, and OUTSIDE over everything beyond the walls
RR_HD uint32_t render_sample_ego(const DrawList &dl, int nr, int nb, float W, float H, uint32_t goal_grumpy, uint32_t goal_happy, float x, float y) {
    uint32_t col = RENDER_BACKGROUND;
    if (x + y <= 240.0f) col = goal_grumpy;
    if ((W - x) + (H - y) <= 240.0f) col = goal_happy;
    for (int r = 0; r < nr; r++) {
        const float dx = x - dl.rx[r], dy = y - dl.ry[r], c = dl.rc[r], s = dl.rs[r];
        const float u = dx * c + dy * s, v = dy * c - dx * s;
        const float au = fabsf(u), av = fabsf(v);
        if (au <= 10.0f && av <= 20.0f) col = (au > 9.0f || av > 19.0f) ? RENDER_BLACK : (u > 7.0f ? RENDER_FRONT : dl.rcol[r]);
    }
    for (int b = 0; b < nb; b++) {
        const float dx = x - dl.bx[b], dy = y - dl.by[b];
        const float d2 = dx * dx + dy * dy;
        if (d2 <= 49.0f) col = d2 > 36.0f ? RENDER_BLACK : dl.bcol[b];
    }
    if (x < 0.0f || x > W || y < 0.0f || y > H) col = RENDER_OUTSIDE;
    return col;
}

// pixel (i, j) of the viewer's frame: p to the right, q downwards, the front up
RR_HD uint32_t render_pixel_ego(const DrawList &dl, int nr, int nb, const EgoView &V, const EgoCamera &cam, int i, int j) {
    const int S = V.S;
    uint32_t sr = 0, sg = 0, sb = 0;
    for (int b = 0; b < S; b++) {
        const float q = ((float)(j * S + b) + 0.5f) * V.f - V.hy;
        const float fwd = V.ahead - q;
        for (int a = 0; a < S; a++) {
            const float p = ((float)(i * S + a) + 0.5f) * V.f - V.hx;
            const float x = cam.cx + (fwd * cam.c - p * cam.s), y = cam.cy + (fwd * cam.s + p * cam.c);
            const uint32_t c = render_sample_ego(dl, nr, nb, V.W, V.H, cam.goal_grumpy, cam.goal_happy, x, y);
            sr += c & 255u; sg += (c >> 8) & 255u; sb += c >> 16;
        }
    }
    const uint32_t k = (uint32_t)(S * S), h = k / 2;
    return render_rgb((sr + h) / k, (sg + h) / k, (sb + h) / k);
}

// the three dwords of quad q: interleaved, render_quad's r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (consecutive); planar, r0 r1 r2 r3 |
// g0 g1 g2 g3 | b0 b1 b2 b3 (dword q of each of the frame's three planes).  valid = false: all zero
RR_HD void render_quad_ego(const DrawList &dl, int nr, int nb, const EgoView &V, const EgoCamera &cam, bool valid, size_t q, uint32_t &w0,
                           uint32_t &w1, uint32_t &w2) {
    w0 = 0; w1 = 0; w2 = 0;
    if (!valid) return;
    const int qpr = V.width / RENDER_QUAD;
    const int j = (int)(q / (size_t)qpr), i0 = (int)(q % (size_t)qpr) * RENDER_QUAD;
    const uint32_t p0 = render_pixel_ego(dl, nr, nb, V, cam, i0, j), p1 = render_pixel_ego(dl, nr, nb, V, cam, i0 + 1, j),
                   p2 = render_pixel_ego(dl, nr, nb, V, cam, i0 + 2, j), p3 = render_pixel_ego(dl, nr, nb, V, cam, i0 + 3, j);
    if (V.flags & RENDER_EGO_PLANAR) {
        w0 = (p0 & 255u) | ((p1 & 255u) << 8) | ((p2 & 255u) << 16) | (p3 << 24);
        w1 = ((p0 >> 8) & 255u) | (p1 & 0xFF00u) | ((p2 & 0xFF00u) << 8) | ((p3 & 0xFF00u) << 16);
        w2 = (p0 >> 16) | ((p1 >> 16) << 8) | (p2 & 0xFF0000u) | ((p3 >> 16) << 24);
    } else {
        w0 = p0 | (p1 << 24);
        w1 = (p1 >> 8) | (p2 << 16);
        w2 = (p2 >> 16) | (p3 << 8);
    }
}
// where the three dwords of quad q go, as dword offsets into a frame of `quads` quads
RR_HD void render_quad_ego_at(int flags, size_t quads, size_t q, size_t &o0, size_t &o1, size_t &o2) {
    if (flags & RENDER_EGO_PLANAR) { o0 = q; o1 = quads + q; o2 = 2 * quads + q; }
    else { o0 = 3 * q; o1 = 3 * q + 1; o2 = 3 * q + 2; }
}

#if defined(__HIPCC__)
// grid: x = ceil(width * height / 4 / 256) blocks of a frame, y = frames frame0 .. frame0 + gridDim.y - 1.  rgb: 4-byte aligned.
__global__ __launch_bounds__(RENDER_THREADS) void k_render(RenderLayout L, RenderView V, const void *recs, int n, const int32_t *arenas,
                                                          size_t frame0, uint8_t *rgb) {
    __shared__ DrawList dl;
    const size_t frame = frame0 + blockIdx.y;
    size_t arena;
    const bool valid = render_arena_of(arenas, frame, n, arena); // uniform over the block
    if (valid) render_build(L, render_record(L, recs, arena), (int)threadIdx.x, dl);
    __syncthreads();
    const size_t quads = (size_t)V.width * (size_t)V.height / RENDER_QUAD;
    const size_t q = (size_t)blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (q >= quads) return;
    uint32_t w0, w1, w2;
    render_quad(dl, L.nr, L.nb, V, valid, q, w0, w1, w2);
    uint32_t *out = reinterpret_cast<uint32_t *>(rgb + frame * quads * 12) + q * 3;
    out[0] = w0; out[1] = w1; out[2] = w2;
}

// the same grid as k_render; robots: the viewing robot of every frame (device pointer, or null: robot 0)
__global__ __launch_bounds__(RENDER_THREADS) void k_render_ego(RenderLayout L, EgoView V, const void *recs, int n, const int32_t *arenas,
                                                              const int32_t *robots, size_t frame0, uint8_t *rgb) {
    __shared__ DrawList dl;
    const size_t frame = frame0 + blockIdx.y;
    size_t arena;
    int viewer;
    bool valid = render_arena_of(arenas, frame, n, arena); // uniform over the block, like everything up to the camera
    valid = render_viewer_of(robots, frame, L.nr, viewer) && valid;
    const bool swap = render_ego_swap(L, V.flags, viewer);
    if (valid) render_build_ego(L, render_record(L, recs, arena), (int)threadIdx.x, swap, dl);
    __syncthreads();
    EgoCamera cam = {};
    if (valid) valid = render_camera(dl, viewer, swap, cam);
    const size_t quads = (size_t)V.width * (size_t)V.height / RENDER_QUAD;
    const size_t q = (size_t)blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (q >= quads) return;
    uint32_t w0, w1, w2;
    render_quad_ego(dl, L.nr, L.nb, V, cam, valid, q, w0, w1, w2);
    size_t o0, o1, o2;
    render_quad_ego_at(V.flags, quads, q, o0, o1, o2);
    uint32_t *out = reinterpret_cast<uint32_t *>(rgb + frame * quads * 12);
    out[o0] = w0; out[o1] = w1; out[o2] = w2;
}
#endif

} // namespace rr
