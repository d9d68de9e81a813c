// vokselis.hpp -- headless C++ host above the C-ABI (include/vokselis_hip.h), restating the public
// surface of the reference crate (src/lib.rs:13-18,37-49): Camera, CameraUniform, Uniform,
// HdrBackBuffer, VolumeTexture, Context, Demo, run -- same names, argument meaning and call order.
// The reference host is Rust; this image has no Rust toolchain, so the compiled host is C++17.
// Window, input, hot reload and the present pass are out of scope.
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vokselis_hip.h"

namespace vokselis {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error("vokselis_hip error " + std::to_string(c) + ": " + m), code(c) {}
};

inline void check(vk_ctx *ctx, int rc) {
    if (rc != VK_OK) {
        const char *m = vk_last_error(ctx);
        throw Error(rc, m ? m : "");
    }
}

// src/utils/mod.rs:15-18
inline uint32_t dispatch_optimal(uint32_t len, uint32_t subgroup_size) {
    uint32_t padded = (subgroup_size - len % subgroup_size) % subgroup_size;
    return (len + padded) / subgroup_size;
}

// src/utils/mod.rs:91-118 (the reference's spelling)
struct ImageDimentions {
    uint32_t width, height, unpadded_bytes_per_row, padded_bytes_per_row;
    ImageDimentions(uint32_t w, uint32_t h, uint32_t align) {
        height = h - (h % 2);
        width = w - (w % 2);
        unpadded_bytes_per_row = width * 4;
        uint32_t row_padding = (align - unpadded_bytes_per_row % align) % align;
        padded_bytes_per_row = unpadded_bytes_per_row + row_padding;
    }
    uint64_t linear_size() const { return (uint64_t)padded_bytes_per_row * height; }
};

// ---- glam 0.20.5 pieces used by src/camera.rs (column-major Mat4) --------------------------------
struct Vec3 { float x, y, z; };
inline Vec3 operator-(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline Vec3 operator*(float s, Vec3 v) { return {s * v.x, s * v.y, s * v.z}; }
inline float dot(Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline Vec3 normalize(Vec3 v) { float l = std::sqrt(dot(v, v)); return {v.x / l, v.y / l, v.z / l}; }

struct Mat4 {
    float m[16];  // column-major: m[c*4 + r]
    static Mat4 look_at_rh(Vec3 eye, Vec3 center, Vec3 up) {
        Vec3 f = normalize(center - eye), s = normalize(cross(f, up)), u = cross(s, f);
        return {{s.x, u.x, -f.x, 0, s.y, u.y, -f.y, 0, s.z, u.z, -f.z, 0, -dot(s, eye), -dot(u, eye), dot(f, eye), 1}};
    }
    static Mat4 perspective_rh(float fovy, float aspect, float z_near, float z_far) {  // depth 0..1
        float sn = std::sin(0.5f * fovy), cs = std::cos(0.5f * fovy);
        float h = cs / sn, w = h / aspect, r = z_far / (z_near - z_far);
        return {{w, 0, 0, 0, 0, h, 0, 0, 0, 0, r, -1, 0, 0, r * z_near, 0}};
    }
    Mat4 operator*(const Mat4 &b) const {
        Mat4 o{};
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++) {
                float s = m[r] * b.m[c * 4];
                s = s + m[4 + r] * b.m[c * 4 + 1];
                s = s + m[8 + r] * b.m[c * 4 + 2];
                s = s + m[12 + r] * b.m[c * 4 + 3];
                o.m[c * 4 + r] = s;
            }
        return o;
    }
    // General inverse by cofactors, binary32, products and sums left to right as written: the one order every host
    // of this build uses (vokselis_amd/camera.py writes the same expressions), so that the same orbit gives the
    // same 144 bytes everywhere.  glam's own SIMD order cannot be reproduced offline.
    Mat4 inverse() const {
        float a[16];
        a[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
        a[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
        a[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
        a[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
        a[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
        a[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
        a[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
        a[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
        a[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
        a[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
        a[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
        a[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
        a[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
        a[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
        a[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
        a[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
        const float det = m[0] * a[0] + m[1] * a[4] + m[2] * a[8] + m[3] * a[12];
        const float rdet = 1.0f / det;
        Mat4 o{};
        for (int i = 0; i < 16; i++) o.m[i] = a[i] * rdet;
        return o;
    }
    static Mat4 identity() { return {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}}; }
};

// src/camera.rs:5-21
struct CameraUniform {
    float view_position[4] = {0, 0, 0, 0};
    float proj_view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float inv_proj[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};
static_assert(sizeof(CameraUniform) == 144, "CameraUniform is 144 bytes (src/camera.rs:5-11)");

// src/camera.rs:74-172
class Camera {
  public:
    static constexpr float ZFAR = 100.f, ZNEAR = 0.1f, FOVY = 3.14159265358979323846f / 2.0f;
    float zoom, pitch, yaw, aspect;
    Vec3 target, eye{0, 0, 0}, up{0, 1, 0};
    bool updated = false;

    Camera(float zoom_, float pitch_, float yaw_, Vec3 target_, float aspect_)
        : zoom(zoom_), pitch(pitch_), yaw(yaw_), aspect(aspect_), target(target_) { fix_eye(); }
    Mat4 build_projection_view_matrix() const {
        return Mat4::perspective_rh(FOVY, aspect, ZNEAR, ZFAR) * Mat4::look_at_rh(eye, target, up);
    }
    void set_zoom(float z) { zoom = std::fmin(std::fmax(z, 0.3f), ZFAR / 2.f); fix_eye(); updated = true; }
    void add_zoom(float d) { set_zoom(zoom + d); }
    void set_pitch(float p) {
        const float eps = 1.1920929e-7f, half_pi = 3.14159265358979323846f / 2.0f;
        pitch = std::fmin(std::fmax(p, -half_pi + eps), half_pi - eps); fix_eye(); updated = true;
    }
    void add_pitch(float d) { set_pitch(pitch + d); }
    void set_yaw(float y) { yaw = y; fix_eye(); updated = true; }
    void add_yaw(float d) { set_yaw(yaw + d); }
    void set_aspect(uint32_t w, uint32_t h) { aspect = (float)w / (float)h; updated = true; }
    CameraUniform get_proj_view_matrix() const {
        CameraUniform u;
        Mat4 pv = build_projection_view_matrix(), inv = pv.inverse();
        u.view_position[0] = eye.x; u.view_position[1] = eye.y; u.view_position[2] = eye.z; u.view_position[3] = 1.0f;
        std::memcpy(u.proj_view, pv.m, 64);
        std::memcpy(u.inv_proj, inv.m, 64);
        return u;
    }

  private:
    void fix_eye() {
        float pc = std::cos(pitch);
        eye = target - zoom * Vec3{std::sin(yaw) * pc, std::sin(pitch), std::cos(yaw) * pc};
    }
};

// src/context/global_ubo.rs:52-81
struct Uniform {
    float pos[3] = {0, 0, 0};
    uint32_t frame = 0;
    float resolution[2] = {1920.0f, 780.f};
    float mouse[2] = {0, 0};
    uint32_t mouse_pressed = 0;
    float time = 0.f;
    float time_delta = 1.f / 60.f;
    float _padding = 0.f;
};
static_assert(sizeof(Uniform) == 48, "Uniform is 48 bytes (src/context/global_ubo.rs:52-65)");
static_assert(sizeof(vk_isosurface) == 20, "vk_isosurface is 20 bytes (vk_set_isosurface)");
static_assert(sizeof(vk_clip_box) == 24, "vk_clip_box is 24 bytes (vk_set_clip_box)");
static_assert(sizeof(vk_shadows) == 8, "vk_shadows is 8 bytes (vk_set_shadows)");
static_assert(sizeof(vk_hit) == 36, "vk_hit is 36 bytes (vk_pick)");
static_assert(sizeof(vk_slice) == 56 && sizeof(vk_slice_sample) == 20, "vk_slice is 56 bytes, vk_slice_sample 20 (vk_render_slice, vk_slice_probe)");
static_assert(sizeof(vk_histogram) == 16 && sizeof(vk_voxel_box) == 24 && sizeof(vk_volume_stats) == 72, "vk_histogram is 16 bytes, vk_voxel_box 24, vk_volume_stats 72 (vk_volume_histogram)");

static_assert(sizeof(vk_mesh_request) == 8, "vk_mesh_request is 8 bytes (vk_extract_isosurface)");
static_assert(sizeof(struct vk_volume_filter) == 176, "struct vk_volume_filter is 176 bytes (vk_volume_filter)");

static_assert(sizeof(vk_label_request) == 232 && sizeof(vk_component) == 40 && sizeof(vk_label_result) == 32, "vk_label_request is 232 bytes, vk_component 40, vk_label_result 32 (vk_label_components)");

// What Context::label_components returns: the components in id order (id k + 1 at index k), the totals, and the labels when asked for.
struct Components {
    std::vector<vk_component> table;
    vk_label_result totals{};
    std::vector<uint32_t> labels;  // nx ny nz, x fastest, 0: background; empty unless asked for
    // the ids of the min(k, n) largest components: by size descending, then by first voxel -- VK_LABEL_KEEP_LARGEST's order
    std::vector<uint64_t> largest(size_t k) const {
        std::vector<uint64_t> ids(table.size());
        for (size_t i = 0; i < ids.size(); i++) ids[i] = i + 1;
        std::stable_sort(ids.begin(), ids.end(), [&](uint64_t a, uint64_t b) { return table[a - 1].n_voxels > table[b - 1].n_voxels; });
        ids.resize(std::min(k, ids.size()));
        return ids;
    }
};
static_assert(sizeof(vk_split_request) == 40 && sizeof(vk_split_result) == 64, "vk_split_request is 40 bytes, vk_split_result 64 (vk_split_components)");
// What Context::split_components returns: the regions in id order (`first` is a region's anchor), the totals, and the labels when asked for.
struct Regions {
    std::vector<vk_component> table;
    vk_split_result totals{};
    std::vector<uint32_t> labels;  // nx ny nz, x fastest, 0: off the set; empty unless asked for
    // the ids of the min(k, table.size()) largest regions of the table: by size descending, then by anchor
    std::vector<uint64_t> largest(size_t k) const {
        std::vector<uint64_t> ids(table.size());
        for (size_t i = 0; i < ids.size(); i++) ids[i] = i + 1;
        std::stable_sort(ids.begin(), ids.end(), [&](uint64_t a, uint64_t b) { return table[a - 1].n_voxels > table[b - 1].n_voxels; });
        ids.resize(std::min(k, ids.size()));
        return ids;
    }
};
static_assert(sizeof(vk_measure_request) == 24 && sizeof(vk_region) == 192 && sizeof(vk_measure_result) == 32, "vk_measure_request is 24 bytes, vk_region 192, vk_measure_result 32 (vk_measure_components)");
// What Context::measure_components returns: the regions' exact integer records in id order (id k + 1 at index k), the totals, the volume's
// dimensions, and the quantities derived from a record in double: the 128-bit fields are joined in __int128, a quotient is taken once.
// An empty region (an id no voxel carries) gives NaN wherever a quotient has no meaning.  k below is an index into `table`: id - 1.
struct Measurements {
    std::vector<vk_region> table;
    vk_measure_result totals{};
    uint32_t dims[3] = {0, 0, 0};
    std::vector<uint64_t> largest(size_t k) const {
        std::vector<uint64_t> ids(table.size());
        for (size_t i = 0; i < ids.size(); i++) ids[i] = i + 1;
        std::stable_sort(ids.begin(), ids.end(), [&](uint64_t a, uint64_t b) { return table[a - 1].n_voxels > table[b - 1].n_voxels; });
        ids.resize(std::min(k, ids.size()));
        return ids;
    }
    // the mean voxel index (x, y, z); centroid_unit: (c + 0.5) / dims, the unit-cube convention of the mesh and of vk_hit.pos
    std::array<double, 3> centroid(size_t k) const {
        const vk_region &r = table[k];
        const double n = (double)r.n_voxels;
        return {r.n_voxels ? (double)r.sum_x / n : NAN, r.n_voxels ? (double)r.sum_y / n : NAN, r.n_voxels ? (double)r.sum_z / n : NAN};
    }
    std::array<double, 3> centroid_unit(size_t k) const {
        const std::array<double, 3> c = centroid(k);
        return {(c[0] + 0.5) / dims[0], (c[1] + 0.5) / dims[1], (c[2] + 0.5) / dims[2]};
    }
    // the covariance of the voxel positions (population form) in the units of spacing (nullptr: 1 1 1): (n S_ab - S_a S_b) / n^2 with the
    // numerator exact in __int128 (it fits whenever n times the largest dimension stays below 2^63: every volume that fits a device)
    std::array<std::array<double, 3>, 3> covariance(size_t k, const double *spacing = nullptr) const {
        const vk_region &r = table[k];
        const uint64_t s[3] = {r.sum_x, r.sum_y, r.sum_z}, p[3][3] = {{r.sum_xx, r.sum_xy, r.sum_xz}, {r.sum_xy, r.sum_yy, r.sum_yz}, {r.sum_xz, r.sum_yz, r.sum_zz}};
        std::array<std::array<double, 3>, 3> c{};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const __int128 num = (__int128)r.n_voxels * p[a][b] - (__int128)s[a] * s[b];
                c[a][b] = r.n_voxels ? (double)num / ((double)r.n_voxels * (double)r.n_voxels) * (spacing ? spacing[a] * spacing[b] : 1.0) : NAN;
            }
        return c;
    }
    // the covariance's eigenvalues, descending, and their unit eigenvectors (vectors[j] belongs to values[j]): cyclic Jacobi sweeps of the 3 x 3 matrix
    void principal_axes(size_t k, const double *spacing, double values[3], double vectors[3][3]) const {
        std::array<std::array<double, 3>, 3> a = covariance(k, spacing);
        double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int sweep = 0; sweep < 32 && std::isfinite(a[0][0]); sweep++) {
            const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
            if (off <= 1e-300 || off <= 1e-17 * (std::fabs(a[0][0]) + std::fabs(a[1][1]) + std::fabs(a[2][2]))) break;
            for (int p = 0; p < 2; p++)
                for (int q = p + 1; q < 3; q++) {
                    if (a[p][q] == 0.0) continue;
                    const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0)), c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                    for (int i = 0; i < 3; i++) { const double x = a[i][p], y = a[i][q]; a[i][p] = c * x - sn * y; a[i][q] = sn * x + c * y; }
                    for (int i = 0; i < 3; i++) { const double x = a[p][i], y = a[q][i]; a[p][i] = c * x - sn * y; a[q][i] = sn * x + c * y; }
                    for (int i = 0; i < 3; i++) { const double x = v[i][p], y = v[i][q]; v[i][p] = c * x - sn * y; v[i][q] = sn * x + c * y; }
                }
        }
        int order[3] = {0, 1, 2};
        std::sort(order, order + 3, [&](int x, int y) { return a[x][x] > a[y][y]; });
        for (int j = 0; j < 3; j++) {
            values[j] = a[order[j]][order[j]];
            for (int i = 0; i < 3; i++) vectors[j][i] = std::isfinite(values[j]) ? v[i][order[j]] : NAN;
        }
    }
    // the full axes, longest first, of the uniform ellipsoid that has the region's covariance: 2 sqrt(5 lambda)
    std::array<double, 3> principal_lengths(size_t k, const double *spacing = nullptr) const {
        double w[3], v[3][3];
        principal_axes(k, spacing, w, v);
        return {2.0 * std::sqrt(5.0 * std::max(w[0], 0.0)), 2.0 * std::sqrt(5.0 * std::max(w[1], 0.0)), 2.0 * std::sqrt(5.0 * std::max(w[2], 0.0))};
    }
    double volume(size_t k, const double *spacing = nullptr) const { return (double)table[k].n_voxels * (spacing ? spacing[0] * spacing[1] * spacing[2] : 1.0); }
    double equivalent_diameter(size_t k, const double *spacing = nullptr) const { return std::cbrt(6.0 * volume(k, spacing) / 3.14159265358979323846); }
    // the area of the exposed voxel faces, faces . (sy sz, sx sz, sx sy): the voxel staircase's surface, an overestimate for a smooth shape
    double surface_area(size_t k, const double *spacing = nullptr) const {
        const vk_region &r = table[k];
        const double sx = spacing ? spacing[0] : 1.0, sy = spacing ? spacing[1] : 1.0, sz = spacing ? spacing[2] : 1.0;
        return (double)r.faces[0] * sy * sz + (double)r.faces[1] * sx * sz + (double)r.faces[2] * sx * sy;
    }
    bool touches_border(size_t k) const {
        const vk_region &r = table[k];
        return r.n_voxels && (r.box.x0 == 0 || r.box.y0 == 0 || r.box.z0 == 0 || r.box.x1 == dims[0] || r.box.y1 == dims[1] || r.box.z1 == dims[2]);
    }
    // intensity in sample values (q / scale), over the finite voxels
    uint64_t n_finite(size_t k) const { return table[k].n_voxels - table[k].n_nonfinite; }
    double mean(size_t k) const {
        const vk_region &r = table[k];
        const __int128 q = ((__int128)r.sum_q_hi << 64) + (__int128)r.sum_q_lo;
        return n_finite(k) ? (double)q / ((double)n_finite(k) * (double)totals.scale) : NAN;
    }
    // (m sum q^2 - (sum q)^2) / (m scale)^2, exact in 128 bits where the products fit (always for the integer formats), else in long double
    double variance(size_t k) const {
        const vk_region &r = table[k];
        const uint64_t m = n_finite(k);
        if (!m) return NAN;
        const __int128 q = ((__int128)r.sum_q_hi << 64) + (__int128)r.sum_q_lo;
        const unsigned __int128 qq = ((unsigned __int128)r.sum_qq_hi << 64) + r.sum_qq_lo, aq = (unsigned __int128)(q < 0 ? -q : q);
        unsigned __int128 left, right;
        const double den = ((double)m * (double)totals.scale) * ((double)m * (double)totals.scale);
        if (!__builtin_mul_overflow(qq, (unsigned __int128)m, &left) && !__builtin_mul_overflow(aq, aq, &right)) return (double)(left - right) / den;  // left >= right (Cauchy-Schwarz)
        const long double mean_q = (long double)q / (long double)m, ms = (long double)qq / (long double)m - mean_q * mean_q;
        return (double)(ms > 0 ? ms : 0) / ((double)totals.scale * (double)totals.scale);
    }
    double stddev(size_t k) const { return std::sqrt(variance(k)); }
    double min(size_t k) const { return n_finite(k) ? (double)table[k].q_min / (double)totals.scale : NAN; }
    double max(size_t k) const { return n_finite(k) ? (double)table[k].q_max / (double)totals.scale : NAN; }
    // one line per region: id, voxels, first, box, centroid, volume, equivalent diameter, principal lengths, mean, std, min, max, nonfinite voxels, faces, area, border
    void to_csv(const std::string &path, const double *spacing = nullptr) const {
        std::FILE *f = std::fopen(path.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + path);
        std::fprintf(f, "id,n_voxels,first,x0,y0,z0,x1,y1,z1,cx,cy,cz,volume,equivalent_diameter,length_1,length_2,length_3,mean,std,min,max,n_nonfinite,faces_x,faces_y,faces_z,surface_area,touches_border\n");
        for (size_t k = 0; k < table.size(); k++) {
            const vk_region &r = table[k];
            const std::array<double, 3> c = centroid(k), l = principal_lengths(k, spacing);
            std::fprintf(f, "%zu,%llu,%llu,%u,%u,%u,%u,%u,%u,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%llu,%llu,%llu,%llu,%.17g,%d\n", k + 1, (unsigned long long)r.n_voxels,
                         (unsigned long long)r.first, r.box.x0, r.box.y0, r.box.z0, r.box.x1, r.box.y1, r.box.z1, c[0], c[1], c[2], volume(k, spacing), equivalent_diameter(k, spacing), l[0], l[1], l[2],
                         mean(k), stddev(k), min(k), max(k), (unsigned long long)r.n_nonfinite, (unsigned long long)r.faces[0], (unsigned long long)r.faces[1], (unsigned long long)r.faces[2],
                         surface_area(k, spacing), touches_border(k) ? 1 : 0);
        }
        if (std::fclose(f) != 0) throw std::runtime_error("cannot write " + path);
    }
};
// The voxel of a volume of nx x ny x nz that holds the unit-cube position pos (vk_hit.pos): min(floor(pos_c n_c), n_c - 1) per axis.
inline std::array<uint32_t, 3> voxel_of(const float pos[3], uint32_t nx, uint32_t ny, uint32_t nz) {
    const uint32_t n[3] = {nx, ny, nz};
    std::array<uint32_t, 3> v{};
    for (int c = 0; c < 3; c++) {
        if (!(pos[c] >= 0.0f && pos[c] <= 1.0f) || n[c] == 0u) throw std::invalid_argument("voxel_of: the position lies outside the unit cube");
        v[c] = std::min((uint32_t)std::floor((double)pos[c] * (double)n[c]), n[c] - 1u);
    }
    return v;
}

// The 2 radius + 1 normalised weights of a Gaussian of `sigma` voxels (vk_filter_gaussian); radius 0: min(6, ceil(3 sigma)).
inline std::vector<float> gaussian_weights(double sigma, uint32_t radius = 0) {
    if (radius == 0u && sigma > 0.0 && sigma < 1e6) radius = (uint32_t)std::min(std::max(std::ceil(3.0 * sigma), 1.0), (double)VK_FILTER_MAX_RADIUS);
    std::vector<float> w(2u * std::min(radius, (uint32_t)VK_FILTER_MAX_RADIUS) + 1u, 0.0f);
    check(nullptr, vk_filter_gaussian(sigma, radius, w.data()));
    return w;
}

// What Context::volume_histogram returns: the counts over the domain and the region's statistics (on the kernel's scale; stats.scale divides it out).
struct Histogram {
    std::vector<uint64_t> counts;
    float lo = 0.0f, hi = 1.0f;
    vk_volume_stats stats{};
    // The window that holds the percentiles p_lo .. p_hi of the counted texels (vk_histogram_window): a domain for set_transfer_function.
    std::pair<float, float> window(double p_lo, double p_hi) const {
        float a = 0.0f, b = 0.0f;
        check(nullptr, vk_histogram_window(counts.data(), (uint32_t)counts.size(), lo, hi, p_lo, p_hi, &a, &b));
        return {a, b};
    }
};

// src/context/hdr_backbuffer.rs:10-11
struct HdrBackBuffer {
    static constexpr uint32_t DEFAULT_W = 1280, DEFAULT_H = 720;
    uint32_t width = DEFAULT_W, height = DEFAULT_H;
    int format = VK_OUT_RGBA16F;
};

// src/utils/frame_counter.rs
struct FrameCounter {
    uint32_t frame_count = 0;
    double accum_time = 0, delta = 1.0 / 60.0;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    float time_delta() const { return (float)delta; }
    double record() {
        auto now = std::chrono::steady_clock::now();
        delta = std::chrono::duration<double>(now - last).count();
        last = now; accum_time += delta; frame_count++;
        return delta;
    }
};

// src/context.rs:38-67,225-249 -- headless
class Context {
  public:
    Camera camera;
    Uniform global_uniform;
    HdrBackBuffer render_backbuffer;
    uint32_t width, height;
    // fuse_present: when the window has the backbuffer's size, RaycastPipeline::record presents from the pass's own epilogue
    // (VK_RENDER_PRESENT) and the render() that follows records nothing: demo.render + context.render (src/lib.rs:178-182) in one launch
    bool fuse_present = false;
    bool pass_presented = false;

    Context(uint32_t w, uint32_t h, const Camera *cam = nullptr, int device = 0, HdrBackBuffer bb = HdrBackBuffer())
        : camera(cam ? *cam : Camera(1.f, 0.5f, 1.f, {0.f, 0.f, 0.f}, (float)w / (float)h)), render_backbuffer(bb), width(w), height(h) {
        int rc = vk_ctx_create(device, &ctx_);
        if (rc != VK_OK) throw Error(rc, vk_last_error(nullptr));
        check(ctx_, vk_backbuffer_resize(ctx_, bb.width, bb.height, bb.format));
        timeline_ = std::chrono::steady_clock::now();
    }
    ~Context() { if (ctx_) vk_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    vk_ctx *handle() const { return ctx_; }

    // Context::update: uniform every frame, camera when `updated` -- and on the first frame (F10)
    void update(const FrameCounter &fc) {
        global_uniform.time = std::chrono::duration<float>(std::chrono::steady_clock::now() - timeline_).count();
        global_uniform.time_delta = fc.time_delta();
        global_uniform.frame = fc.frame_count;
        global_uniform.resolution[0] = (float)width; global_uniform.resolution[1] = (float)height;
        check(ctx_, vk_set_uniform(ctx_, &global_uniform));
        if (camera.updated || first_frame_) {
            CameraUniform cu = camera.get_proj_view_matrix();
            check(ctx_, vk_set_camera(ctx_, &cu));
            camera.updated = false; first_frame_ = false;
        }
    }
    void resize(uint32_t w, uint32_t h) { width = w; height = h; camera.set_aspect(w, h); }  // context.rs:238-249
    void sync() { check(ctx_, vk_ctx_sync(ctx_)); }
    // Runtime transfer function of NAIVE_TRILINEAR (vk_set_transfer_function): n RGBA entries over the sample values [lo, hi];
    // rgba == nullptr resets to the built-in transfer (raycast_naive.wgsl:104-110).
    void set_transfer_function(const float *rgba, uint32_t n, float lo = 0.0f, float hi = 1.0f) {
        check(ctx_, vk_set_transfer_function(ctx_, rgba, n, lo, hi));
    }
    // Projection of NAIVE_TRILINEAR (vk_set_projection): VK_PROJ_MAX, a maximum-intensity projection over the table's window, or VK_PROJ_COMPOSITE.
    void set_projection(int projection) { check(ctx_, vk_set_projection(ctx_, projection)); }
    int projection() const { int p = VK_PROJ_COMPOSITE; check(ctx_, vk_get_projection(ctx_, &p)); return p; }
    // First-hit isosurface rendering of NAIVE_TRILINEAR (vk_set_isosurface); nullptr turns it off.  While set, table and projection are ignored (and kept).
    void set_isosurface(const vk_isosurface *iso) { check(ctx_, vk_set_isosurface(ctx_, iso)); }
    bool isosurface(vk_isosurface *out = nullptr) const { int on = 0; check(ctx_, vk_get_isosurface(ctx_, out, &on)); return on != 0; }
    // Gradient lighting of the table march (vk_set_lighting); nullptr turns it off.
    void set_lighting(const vk_lighting *light) { check(ctx_, vk_set_lighting(ctx_, light)); }
    // Light-direction shadows of the lit isosurface (vk_set_shadows); nullptr turns them off.  Ignored unless an isosurface and a light that is
    // not a headlight are set.
    void set_shadows(const vk_shadows *s) { check(ctx_, vk_set_shadows(ctx_, s)); }
    bool shadows(vk_shadows *out = nullptr) const { int on = 0; check(ctx_, vk_get_shadows(ctx_, out, &on)); return on != 0; }
    // Clip box (cut-away) of the table, lit, MAX and isosurface marches, in unit-cube coordinates (vk_set_clip_box); nullptr turns it off.
    void set_clip_box(const vk_clip_box *box) { check(ctx_, vk_set_clip_box(ctx_, box)); }
    bool clip_box(vk_clip_box *out = nullptr) const { int on = 0; check(ctx_, vk_get_clip_box(ctx_, out, &on)); return on != 0; }
    // The geometry pass of the first-hit isosurface (vk_render_geometry): per pixel the refined crossing, its distance along the ray, the raw gradient
    // and the sample there, into the current frame slot's geometry surface; asynchronous.  Needs an isosurface; lighting, shadows, table and
    // projection have no influence.  flags: VK_RENDER_NO_SKIP, _SAFE, _FORCE_SKIP, _PROBE_ALWAYS.
    void render_geometry(float dt_scale = 1.0f, uint32_t flags = 0) { check(ctx_, vk_render_geometry(ctx_, 0, 0, render_backbuffer.width, render_backbuffer.height, dt_scale, flags)); }
    void render_geometry_tile(int32_t x, int32_t y, uint32_t w, uint32_t h, float dt_scale = 1.0f, uint32_t flags = 0) { check(ctx_, vk_render_geometry(ctx_, x, y, w, h, dt_scale, flags)); }
    // [height][width][2][4] floats: (q.x, q.y, q.z, t), (g.x, g.y, g.z, x) per pixel; t = +inf: a miss.  Blocks.
    std::vector<float> read_geometry() {
        std::vector<float> out((size_t)render_backbuffer.width * render_backbuffer.height * 8);
        check(ctx_, vk_readback_geometry(ctx_, out.data(), (size_t)render_backbuffer.width * 32));
        return out;
    }
    std::vector<float> frame_geometry(uint64_t id) {  // ... of that frame's slot (vk_frame_readback's rules)
        std::vector<float> out((size_t)render_backbuffer.width * render_backbuffer.height * 8);
        check(ctx_, vk_frame_geometry(ctx_, id, out.data(), (size_t)render_backbuffer.width * 32));
        return out;
    }
    void *geometry_device_ptr() const { void *p = nullptr; check(ctx_, vk_geometry_info(ctx_, nullptr, nullptr, &p)); return p; }  // (does not synchronise)
    // What the ray through pixel (x, y) hits (vk_pick; blocks): hit.hit == 0 for a miss.  The outward normal of a surface entered from below the
    // threshold is -grad / |grad|.
    vk_hit pick(uint32_t x, uint32_t y, float dt_scale = 1.0f) { vk_hit h{}; check(ctx_, vk_pick(ctx_, x, y, dt_scale, &h)); return h; }
    // The slice pass (vk_render_slice): the plane `s` into the backbuffer (or a tile of it) -- the volume filtered at each pixel's position, or a
    // slab of samples reduced by max / min / mean, through the table in force, as sRGB; asynchronous.  No camera; only table and clip box have
    // influence.  values: also write the (x, weight) records into the slot's value surface.
    void render_slice(const vk_slice &s, bool values = false) { check(ctx_, vk_render_slice(ctx_, &s, 0, 0, render_backbuffer.width, render_backbuffer.height, values ? VK_SLICE_VALUES : 0u)); }
    void render_slice_tile(const vk_slice &s, int32_t x, int32_t y, uint32_t w, uint32_t h, bool values = false) { check(ctx_, vk_render_slice(ctx_, &s, x, y, w, h, values ? VK_SLICE_VALUES : 0u)); }
    // [height][width][2] floats: (x, weight) per pixel, weight 0 (and x = +0) outside the box.  Blocks.
    std::vector<float> read_slice_values() {
        std::vector<float> out((size_t)render_backbuffer.width * render_backbuffer.height * 2);
        check(ctx_, vk_readback_slice_values(ctx_, out.data(), (size_t)render_backbuffer.width * 8));
        return out;
    }
    std::vector<float> frame_slice_values(uint64_t id) {  // ... of that frame's slot (vk_frame_readback's rules)
        std::vector<float> out((size_t)render_backbuffer.width * render_backbuffer.height * 2);
        check(ctx_, vk_frame_slice_values(ctx_, id, out.data(), (size_t)render_backbuffer.width * 8));
        return out;
    }
    void *slice_values_device_ptr() const { void *p = nullptr; check(ctx_, vk_slice_values_info(ctx_, nullptr, nullptr, &p)); return p; }  // (does not synchronise)
    // The value under pixel (x, y) of the plane (vk_slice_probe; blocks): inside == 0 where the position lies outside the box.
    vk_slice_sample slice_probe(const vk_slice &s, uint32_t x, uint32_t y) { vk_slice_sample o{}; check(ctx_, vk_slice_probe(ctx_, &s, x, y, &o)); return o; }
    // The histogram of the stored texels over [lo, hi] (sample values) and the statistics of the voxel box (vk_volume_histogram; blocks; changes no
    // state): box == nullptr is the whole volume, or with clip == true the voxels whose centres lie in the clip box in force.
    Histogram volume_histogram(uint32_t bins = 256, float lo = 0.0f, float hi = 1.0f, const vk_voxel_box *box = nullptr, bool clip = false) {
        Histogram h;
        h.lo = lo; h.hi = hi;
        h.counts.assign(bins <= (uint32_t)VK_HIST_MAX_BINS ? bins : 0u, 0u);
        const vk_histogram req = {lo, hi, bins, clip ? (uint32_t)VK_HIST_CLIP_BOX : 0u};
        check(ctx_, vk_volume_histogram(ctx_, &req, box, h.counts.data(), &h.stats));
        return h;
    }
    // The isosurface `stored texel >= iso` (sample values; independent of set_isosurface) as triangles by marching tetrahedra
    // (vk_extract_isosurface; blocks; changes no state): 9 floats per triangle, unit-cube coordinates, normals towards lower values.  box ==
    // nullptr is the whole volume, or with clip == true the voxels whose centres lie in the clip box in force.  A count call, then a fill call.
    std::vector<float> extract_isosurface(float iso, const vk_voxel_box *box = nullptr, bool clip = false) {
        const vk_mesh_request req = {iso, clip ? (uint32_t)VK_MESH_CLIP_BOX : 0u};
        uint64_t n = 0;
        check(ctx_, vk_extract_isosurface(ctx_, &req, box, nullptr, 0, &n));
        std::vector<float> tris((size_t)n * 9u);
        if (n) check(ctx_, vk_extract_isosurface(ctx_, &req, box, tris.data(), n, &n));
        return tris;
    }
    // The volume filter pass (vk_volume_filter): the stored volume through a separable convolution -- wx, wy, wz each empty (the axis is
    // skipped) or 2 r + 1 weights, r <= VK_FILTER_MAX_RADIUS -- into a volume of the same dimensions and format.  install: the result replaces
    // the context's volume in its layout, under the table / projection / isosurface in force (outside frame_begin / frame_end).  dense_out:
    // nullptr, or host memory of nx ny nz elements of the volume's format (the call then blocks).
    void filter_volume(const std::vector<float> &wx, const std::vector<float> &wy, const std::vector<float> &wz, bool install = true, void *dense_out = nullptr) {
        struct vk_volume_filter f{};
        f.op = VK_FILTER_CONVOLVE;
        f.flags = install ? (uint32_t)VK_FILTER_INSTALL : 0u;
        const std::vector<float> *w[3] = {&wx, &wy, &wz};
        for (int a = 0; a < 3; a++) {
            if (w[a]->empty()) continue;
            if (w[a]->size() % 2u == 0u || w[a]->size() < 3u || w[a]->size() > 2u * VK_FILTER_MAX_RADIUS + 1u)
                throw std::invalid_argument("filter_volume: an odd number 2 r + 1 of weights per axis, 1 <= r <= VK_FILTER_MAX_RADIUS (empty: the axis is skipped)");
            f.radius[a] = (uint32_t)(w[a]->size() / 2u);
            for (size_t k = 0; k < w[a]->size(); k++) f.weights[a][k] = (*w[a])[k];
        }
        check(ctx_, vk_volume_filter(ctx_, &f, dense_out));
    }
    // ... with Gaussian weights of (sx, sy, sz) voxels; a sigma of 0 skips its axis
    void smooth_volume(double sx, double sy, double sz, bool install = true, void *dense_out = nullptr) {
        const std::vector<float> none;
        filter_volume(sx != 0.0 ? gaussian_weights(sx) : none, sy != 0.0 ? gaussian_weights(sy) : none, sz != 0.0 ? gaussian_weights(sz) : none, install, dense_out);
    }
    // ... the 3x3x3 median: every texel becomes the 14th smallest of its 27 neighbours
    void median_volume(bool install = true, void *dense_out = nullptr) {
        struct vk_volume_filter f{};
        f.op = VK_FILTER_MEDIAN3;
        f.flags = install ? (uint32_t)VK_FILTER_INSTALL : 0u;
        check(ctx_, vk_volume_filter(ctx_, &f, dense_out));
    }
    // The extents of a pass's voxel box: `box`, else with clip the voxels whose centres lie in the clip box in force, else the volume
    // (vk_resample_output: the library's own rule; an empty box is refused).
    std::array<uint32_t, 3> box_dims(const vk_voxel_box *box = nullptr, bool clip = false) const {
        vk_resample_request req{};
        req.mode = VK_RESAMPLE_NEAREST;
        req.flags = clip ? (uint32_t)VK_RESAMPLE_CLIP_BOX : 0u;
        req.format = VK_RESAMPLE_KEEP_FORMAT;
        vk_resample_result res{};
        check(ctx_, vk_resample_output(ctx_, &req, box, &res));
        return {res.dims[0], res.dims[1], res.dims[2]};
    }
    // The resample pass (vk_volume_resample): the voxel box (box; with clip the clip box's voxels; neither: the whole volume) resampled to
    // dims (nullptr or 0 per axis: the box's extent) by mode = VK_RESAMPLE_NEAREST / _LINEAR / _AREA, into format (VK_RESAMPLE_KEEP_FORMAT:
    // the volume's), under window = {lo, hi} in sample values (nullptr: none).  install: the result replaces the context's volume in
    // `layout` (VK_LAYOUT_AUTO: the current one, PACKED where that cannot hold the new format; outside frame_begin / frame_end).  dense:
    // nullptr, or a vector that is sized to the output and filled.  Needs install or dense.
    vk_resample_result resample_volume(const uint32_t *dims = nullptr, int mode = VK_RESAMPLE_LINEAR, const vk_voxel_box *box = nullptr, bool clip = false,
                                       int format = VK_RESAMPLE_KEEP_FORMAT, const float *window = nullptr, int layout = VK_LAYOUT_AUTO, bool install = true,
                                       std::vector<unsigned char> *dense = nullptr) {
        if (!install && !dense) throw std::invalid_argument("resample_volume: needs install or dense");
        vk_resample_request req{};
        req.mode = mode;
        req.flags = (install ? (uint32_t)VK_RESAMPLE_INSTALL : 0u) | (clip ? (uint32_t)VK_RESAMPLE_CLIP_BOX : 0u) | (window ? (uint32_t)VK_RESAMPLE_WINDOW : 0u);
        for (int a = 0; a < 3; a++) req.dims[a] = dims ? dims[a] : 0u;
        req.format = format;
        req.layout = layout;
        if (window) { req.lo = window[0]; req.hi = window[1]; }
        vk_resample_result res{};
        if (dense) {  // the library says what the call will write, or refuses as the call would
            check(ctx_, vk_resample_output(ctx_, &req, box, &res));
            dense->assign((size_t)res.dims[0] * res.dims[1] * res.dims[2] * (res.format == VK_FMT_R8_UNORM ? 1u : 2u), 0);
        }
        check(ctx_, vk_volume_resample(ctx_, &req, box, dense ? dense->data() : nullptr, &res));
        return res;
    }
    // ... the voxels of a box become the volume, bit for bit (NEAREST at the box's own extents); box == nullptr: the clip box, which is turned
    // off after a successful install -- the crop is what it showed
    vk_resample_result crop_volume(const vk_voxel_box *box, bool install = true, std::vector<unsigned char> *dense = nullptr) {
        const vk_resample_result r = resample_volume(nullptr, VK_RESAMPLE_NEAREST, box, box == nullptr, VK_RESAMPLE_KEEP_FORMAT, nullptr, VK_LAYOUT_AUTO, install, dense);
        if (!box && install) check(ctx_, vk_set_clip_box(ctx_, nullptr));
        return r;
    }
    // ... every output voxel the mean of the factor^3 voxels it covers (AREA to ceil(n / factor) per axis; factor 1 .. VK_RESAMPLE_MAX_RATIO)
    vk_resample_result downsample_volume(uint32_t factor, bool install = true, std::vector<unsigned char> *dense = nullptr) {
        if (factor < 1u) throw std::invalid_argument("downsample_volume: factor >= 1");
        const std::array<uint32_t, 3> bd = box_dims();
        const uint32_t dims[3] = {(bd[0] + factor - 1u) / factor, (bd[1] + factor - 1u) / factor, (bd[2] + factor - 1u) / factor};
        return resample_volume(dims, VK_RESAMPLE_AREA, nullptr, false, VK_RESAMPLE_KEEP_FORMAT, nullptr, VK_LAYOUT_AUTO, install, dense);
    }
    // ... a scan whose voxels measure spacing = {sx, sy, sz} into cubic voxels of the finest of the three: max(1, round(n_c s_c / min(s))) per axis
    vk_resample_result isotropic_volume(const double spacing[3], int mode = VK_RESAMPLE_LINEAR, bool install = true, std::vector<unsigned char> *dense = nullptr) {
        const double m = std::min(spacing[0], std::min(spacing[1], spacing[2]));
        if (!(m > 0.0) || !std::isfinite(spacing[0]) || !std::isfinite(spacing[1]) || !std::isfinite(spacing[2])) throw std::invalid_argument("isotropic_volume: three finite spacings > 0");
        const std::array<uint32_t, 3> bd = box_dims();
        uint32_t dims[3];
        for (int a = 0; a < 3; a++) dims[a] = (uint32_t)std::max(1.0, std::nearbyint((double)bd[a] * spacing[a] / m));
        return resample_volume(dims, mode, nullptr, false, VK_RESAMPLE_KEEP_FORMAT, nullptr, VK_LAYOUT_AUTO, install, dense);
    }
    // Connected components of the voxels whose stored texel lies in [lo, hi] (sample values; vk_label_components; blocks; changes no state):
    // connectivity 6, 18 or 26; box == nullptr: the whole volume, or with clip the clip box in force.  One call with room for 4096
    // components; a second only when there are more.
    Components label_components(float lo, float hi = INFINITY, uint32_t connectivity = 6, const vk_voxel_box *box = nullptr, bool clip = false, bool want_labels = false) {
        vk_label_request req{};
        req.lo = lo; req.hi = hi; req.connectivity = connectivity;
        req.flags = clip ? (uint32_t)VK_LABEL_CLIP_BOX : 0u;
        Components c;
        if (want_labels) {
            uint32_t dims[3] = {0, 0, 0};
            check(ctx_, vk_volume_info(ctx_, dims, nullptr, nullptr, nullptr));
            c.labels.assign((size_t)dims[0] * dims[1] * dims[2], 0u);
        }
        c.table.resize(4096);
        check(ctx_, vk_label_components(ctx_, &req, box, want_labels ? c.labels.data() : nullptr, c.table.data(), c.table.size(), nullptr, &c.totals));
        if (c.totals.n_components > c.table.size()) {
            c.table.resize((size_t)c.totals.n_components);
            check(ctx_, vk_label_components(ctx_, &req, box, nullptr, c.table.data(), c.table.size(), nullptr, &c.totals));
        }
        c.table.resize((size_t)c.totals.n_components);
        return c;
    }
    // ... with a selection: keep = VK_LABEL_KEEP_ALL / _LARGEST (the `count` largest) / _MIN_SIZE (at least `count` voxels) / _SEEDS (the
    // components that hold one of `seeds`, voxels (x, y, z)).  Kept components keep their stored texels, every other voxel becomes `fill`;
    // invert: the other way round.  install: the result replaces the context's volume (outside frame_begin / frame_end).  dense_out: nullptr,
    // or host memory of nx ny nz elements of the volume's format.  Needs install or dense_out.
    vk_label_result keep_components(float lo, float hi, int keep, uint64_t count = 0, const std::vector<std::array<uint32_t, 3>> &seeds = {}, bool invert = false, float fill = 0.0f,
                                    uint32_t connectivity = 6, const vk_voxel_box *box = nullptr, bool clip = false, bool install = true, void *dense_out = nullptr) {
        if (seeds.size() > (size_t)VK_LABEL_MAX_SEEDS) throw std::invalid_argument("keep_components: at most VK_LABEL_MAX_SEEDS seeds");
        if (!install && !dense_out) throw std::invalid_argument("keep_components: needs install or dense_out");
        vk_label_request req{};
        req.lo = lo; req.hi = hi; req.connectivity = connectivity; req.keep = keep; req.count = count; req.fill = fill;
        req.flags = (clip ? (uint32_t)VK_LABEL_CLIP_BOX : 0u) | (install ? (uint32_t)VK_LABEL_INSTALL : 0u) | (invert ? (uint32_t)VK_LABEL_INVERT : 0u);
        req.n_seeds = (uint32_t)seeds.size();
        for (size_t k = 0; k < seeds.size(); k++)
            for (int c = 0; c < 3; c++) req.seeds[k][c] = seeds[k][c];
        vk_label_result res{};
        check(ctx_, vk_label_components(ctx_, &req, box, nullptr, nullptr, 0, dense_out, &res));
        return res;
    }
    // The squared Euclidean distance of every voxel to the set S of voxels whose stored texel lies in [lo, hi] (inside == false: 0 on S) or to
    // its complement (inside: 0 off S), over the integer voxel pitch spacing = {sx, sy, sz} (nullptr: 1 1 1): nx ny nz uint32, x fastest,
    // VK_DIST_INF where the target set is empty (vk_distance_transform; blocks; changes no state).  box / clip restrict S only.
    std::vector<uint32_t> distance_transform(float lo, float hi = INFINITY, bool inside = false, const uint32_t *spacing = nullptr, const vk_voxel_box *box = nullptr, bool clip = false,
                                             vk_distance_result *result = nullptr) {
        vk_distance_request req{};
        req.lo = lo; req.hi = hi; req.op = inside ? VK_DIST_INSIDE : VK_DIST_OUTSIDE;
        req.flags = clip ? (uint32_t)VK_DIST_CLIP_BOX : 0u;
        for (int c = 0; c < 3; c++) req.spacing[c] = spacing ? spacing[c] : 1u;
        uint32_t dims[3] = {0, 0, 0};
        check(ctx_, vk_volume_info(ctx_, dims, nullptr, nullptr, nullptr));
        std::vector<uint32_t> d2((size_t)dims[0] * dims[1] * dims[2], 0u);
        check(ctx_, vk_distance_transform(ctx_, &req, box, d2.data(), nullptr, result));
        return d2;
    }
    // ... and morphology on it: op = VK_DIST_DILATE / _ERODE / _CLOSE / _OPEN by a Euclidean ball of `radius`, in the units of spacing.  A voxel
    // that joins the set becomes fill_in, one that leaves it fill_out, every other voxel keeps its bits.  install: the result replaces the
    // context's volume (outside frame_begin / frame_end).  dense_out: nullptr, or host memory of nx ny nz elements of the volume's format.
    vk_distance_result morph_volume(float lo, float hi, int op, float radius, const uint32_t *spacing = nullptr, float fill_in = 1.0f, float fill_out = 0.0f, const vk_voxel_box *box = nullptr,
                                    bool clip = false, bool install = true, void *dense_out = nullptr) {
        vk_distance_request req{};
        req.lo = lo; req.hi = hi; req.op = op; req.radius = radius; req.fill_in = fill_in; req.fill_out = fill_out;
        req.flags = (clip ? (uint32_t)VK_DIST_CLIP_BOX : 0u) | (install ? (uint32_t)VK_DIST_INSTALL : 0u);
        for (int c = 0; c < 3; c++) req.spacing[c] = spacing ? spacing[c] : 1u;
        vk_distance_result res{};
        check(ctx_, vk_distance_transform(ctx_, &req, box, nullptr, dense_out, &res));
        return res;
    }
    // Split touching objects (vk_split_components; blocks): S = the voxels in [lo, hi] is eroded by `radius` (in the units of the integer pitch
    // spacing, nullptr: 1 1 1), the markers that survive grow back over S, and a voxel beside a region of smaller id becomes fill_out (which
    // must lie outside the range).  The table's `first` is a region's anchor.  install: the cut volume replaces the context's (outside
    // frame_begin / frame_end); dense_out: nullptr, or host memory of nx ny nz elements of the volume's format.  One call with room for
    // 4096 regions; a second, for the table alone, only when there are more and nothing was installed: after an install the context holds
    // the cut volume, so the table then stays at its first 4096 regions and totals.n_regions tells how many there are.
    Regions split_components(float lo, float hi, float radius, const uint32_t *spacing = nullptr, uint32_t connectivity = 6, const vk_voxel_box *box = nullptr, bool clip = false,
                             bool want_labels = false, float fill_out = 0.0f, bool install = false, void *dense_out = nullptr) {
        vk_split_request req{};
        req.lo = lo; req.hi = hi; req.connectivity = connectivity; req.radius = radius; req.fill_out = fill_out;
        req.flags = (clip ? (uint32_t)VK_SPLIT_CLIP_BOX : 0u) | (install ? (uint32_t)VK_SPLIT_INSTALL : 0u);
        for (int c = 0; c < 3; c++) req.spacing[c] = spacing ? spacing[c] : 1u;
        Regions r;
        if (want_labels) {
            uint32_t dims[3] = {0, 0, 0};
            check(ctx_, vk_volume_info(ctx_, dims, nullptr, nullptr, nullptr));
            r.labels.assign((size_t)dims[0] * dims[1] * dims[2], 0u);
        }
        r.table.resize(4096);
        check(ctx_, vk_split_components(ctx_, &req, box, want_labels ? r.labels.data() : nullptr, r.table.data(), r.table.size(), dense_out, &r.totals));
        if (r.totals.n_regions > r.table.size() && !install) {
            r.table.resize((size_t)r.totals.n_regions);
            check(ctx_, vk_split_components(ctx_, &req, box, nullptr, r.table.data(), r.table.size(), nullptr, &r.totals));
        }
        r.table.resize((size_t)std::min<uint64_t>(r.totals.n_regions, r.table.size()));
        return r;
    }
    // Measure labelled regions (vk_measure_components; blocks; changes no state): one exact integer record per region and what derives from
    // it (Measurements).  labels nullptr: the regions are label_components' components of [lo, hi] under `connectivity` inside box / the
    // clip box -- after split_components(install) the split regions; the label array stays on the device.  labels: nx ny nz ids, x fastest,
    // 0 background (label_components' or split_components' labels, or the caller's own); the regions are 1 .. max_label and lo, hi,
    // connectivity and box are not used.  One call with room for 4096 regions, a second only when there are more.
    Measurements measure_components(float lo, float hi = INFINITY, uint32_t connectivity = 6, const vk_voxel_box *box = nullptr, bool clip = false, const uint32_t *labels = nullptr,
                                    uint32_t max_label = 0) {
        vk_measure_request req{};
        if (labels) req.max_label = max_label;
        else { req.lo = lo; req.hi = hi; req.connectivity = connectivity; req.flags = clip ? (uint32_t)VK_MEASURE_CLIP_BOX : 0u; }
        Measurements m;
        check(ctx_, vk_volume_info(ctx_, m.dims, nullptr, nullptr, nullptr));
        m.table.resize(4096);
        check(ctx_, vk_measure_components(ctx_, &req, labels ? nullptr : box, labels, m.table.data(), m.table.size(), &m.totals));
        if (m.totals.n_regions > m.table.size()) {
            m.table.resize((size_t)m.totals.n_regions);
            check(ctx_, vk_measure_components(ctx_, &req, labels ? nullptr : box, labels, m.table.data(), m.table.size(), &m.totals));
        }
        m.table.resize((size_t)m.totals.records_written);
        return m;
    }
    // Local thickness (vk_local_thickness; blocks): for every voxel of S = the voxels in [lo, hi], the squared radius T2 of the largest ball
    // that fits inside S and holds the voxel, over the integer pitch spacing (nullptr: 1 1 1), capped at max_radius^2.  The dense map stores
    // sqrtf(T2) * gain on S (gain 0: automatic, the thickest place stores full scale) and fill_out elsewhere.  install: it replaces the
    // context's volume (outside frame_begin / frame_end); dense_out: nullptr, or host memory of nx ny nz elements of the volume's format;
    // t2_out: nullptr, or nx ny nz uint32.  The thickness a user reads is 2 sqrt(T2): thickness_of.
    vk_thickness_result local_thickness(float lo, float hi = INFINITY, float max_radius = 16.0f, const uint32_t *spacing = nullptr, const vk_voxel_box *box = nullptr, bool clip = false,
                                        float gain = 0.0f, float fill_out = 0.0f, bool install = false, void *dense_out = nullptr, uint32_t *t2_out = nullptr) {
        vk_thickness_request req{};
        req.lo = lo; req.hi = hi; req.max_radius = max_radius; req.gain = gain; req.fill_out = fill_out;
        req.flags = (clip ? (uint32_t)VK_THICK_CLIP_BOX : 0u) | (install ? (uint32_t)VK_THICK_INSTALL : 0u);
        for (int c = 0; c < 3; c++) req.spacing[c] = spacing ? spacing[c] : 1u;
        vk_thickness_result res{};
        check(ctx_, vk_local_thickness(ctx_, &req, box, t2_out, dense_out, &res));
        return res;
    }
    static double thickness_of(uint32_t t2) { return 2.0 * std::sqrt((double)t2); }
    // Geodesic distance (vk_geodesic_distance; blocks): for every voxel of S = the voxels in [lo, hi], the length g of the shortest path inside S
    // from the source set -- the voxels of S on the faces of source_faces (VK_GEO_FACE_*) and the seeds that lie in S -- in units of 1 / VK_GEO_UNIT
    // of the integer pitch spacing (nullptr: 1 1 1), over steps to the 6, 18 or 26 neighbours.  target_faces: the faces whose nearest reached voxel
    // gives target_min (VK_GEO_INF: S does not percolate).  The dense map stores (float)g * gain on a reached voxel (gain 0: automatic, the farthest
    // stores full scale), fill_unreached on the rest of S and fill_out elsewhere.  install: it replaces the context's volume (outside frame_begin /
    // frame_end); dense_out: nullptr, or host memory of nx ny nz elements of the volume's format; g_out: nullptr, or nx ny nz uint32.
    vk_geodesic_result geodesic_distance(float lo, float hi = INFINITY, uint32_t source_faces = VK_GEO_FACE_X0, uint32_t target_faces = 0u, const std::vector<std::array<uint32_t, 3>> &seeds = {},
                                         uint32_t connectivity = 26u, const uint32_t *spacing = nullptr, const vk_voxel_box *box = nullptr, bool clip = false, float gain = 0.0f,
                                         float fill_out = 0.0f, float fill_unreached = 0.0f, bool install = true, void *dense_out = nullptr, uint32_t *g_out = nullptr) {
        if (seeds.size() > (size_t)VK_GEO_MAX_SEEDS) throw std::runtime_error("geodesic_distance: at most VK_GEO_MAX_SEEDS seeds");
        vk_geodesic_request req{};
        req.lo = lo; req.hi = hi; req.connectivity = connectivity; req.gain = gain; req.fill_out = fill_out; req.fill_unreached = fill_unreached;
        req.flags = (clip ? (uint32_t)VK_GEO_CLIP_BOX : 0u) | (install ? (uint32_t)VK_GEO_INSTALL : 0u);
        for (int c = 0; c < 3; c++) req.spacing[c] = spacing ? spacing[c] : 1u;
        req.source_faces = source_faces; req.target_faces = target_faces; req.n_seeds = (uint32_t)seeds.size();
        for (size_t s = 0; s < seeds.size(); s++)
            for (int c = 0; c < 3; c++) req.seeds[s][c] = seeds[s][c];
        vk_geodesic_result res{};
        check(ctx_, vk_geodesic_distance(ctx_, &req, box, g_out, dense_out, &res));
        return res;
    }
    static double geodesic_units(uint32_t g) { return (double)g / (double)VK_GEO_UNIT; }
    // Skeleton (vk_skeletonize; blocks): S = the voxels in [lo, hi] thinned to a one-voxel-wide set with the same pieces, tunnels and cavities, the set
    // 26-connected and the background 6-connected.  mode: VK_SKEL_CURVE keeps line ends (centre lines), VK_SKEL_KERNEL does not (the ultimate homotopic
    // kernel); max_iterations: 0 thins until an iteration deletes nothing.  The dense volume keeps the stored value on the skeleton -- fill_in: nullptr, or
    // the sample value stored there instead -- and stores fill_out elsewhere.  install: it replaces the context's volume (outside frame_begin / frame_end);
    // dense_out: nullptr, or host memory of nx ny nz elements of the volume's format; class_out: nullptr, or nx ny nz bytes (VK_SKEL_OFF .. VK_SKEL_JUNCTION).
    vk_skeleton_result skeletonize(float lo, float hi = INFINITY, uint32_t mode = VK_SKEL_CURVE, uint32_t max_iterations = 0u, const vk_voxel_box *box = nullptr, bool clip = false,
                                   const float *fill_in = nullptr, float fill_out = 0.0f, bool install = true, void *dense_out = nullptr, uint8_t *class_out = nullptr) {
        vk_skeleton_request req{};
        req.lo = lo; req.hi = hi; req.mode = mode; req.max_iterations = max_iterations; req.fill_in = fill_in ? *fill_in : 0.0f; req.fill_out = fill_out;
        req.flags = (clip ? (uint32_t)VK_SKEL_CLIP_BOX : 0u) | (install ? (uint32_t)VK_SKEL_INSTALL : 0u) | (fill_in ? (uint32_t)VK_SKEL_FILL_IN : 0u);
        vk_skeleton_result res{};
        check(ctx_, vk_skeletonize(ctx_, &req, box, class_out, dense_out, &res));
        return res;
    }
    // Steady-state diffusion (vk_steady_diffusion; blocks): the Laplace equation on S = the voxels in [lo, hi], no-flux walls, concentration 1 on the box's first
    // plane along axis (0, 1, 2) and 0 on its last, by red-black over-relaxation in float32 with the integer pitch spacing (nullptr: 1 1 1).  omega: 0 picks
    // the factor from the extent along the axis; sweeps run in blocks of check_every until the largest change of a block's last sweep is <= delta_tol and the
    // two faces' fluxes agree to flux_tol, or until max_sweeps (converged == 0).  The dense map stores c * gain (gain 0: 1) on S and fill_out elsewhere.
    // install (default false: the product is a number): it replaces the context's volume (outside frame_begin / frame_end); dense_out: nullptr, or host
    // memory of nx ny nz elements of the volume's format; c_out: nullptr, or nx ny nz floats (the bits VK_DIFF_OFF off S).
    vk_diffusion_result steady_diffusion(float lo, float hi = INFINITY, uint32_t axis = 2u, const uint32_t *spacing = nullptr, float omega = 0.0f, uint32_t check_every = 32u,
                                         float delta_tol = 1e-5f, float flux_tol = 1e-3f, uint32_t max_sweeps = 20000u, const vk_voxel_box *box = nullptr, bool clip = false, float gain = 0.0f,
                                         float fill_out = 0.0f, bool install = false, void *dense_out = nullptr, float *c_out = nullptr) {
        vk_diffusion_request req{};
        req.lo = lo; req.hi = hi; req.axis = axis; req.omega = omega; req.check_every = check_every; req.max_sweeps = max_sweeps; req.delta_tol = delta_tol; req.flux_tol = flux_tol;
        req.gain = gain; req.fill_out = fill_out;
        req.flags = (clip ? (uint32_t)VK_DIFF_CLIP_BOX : 0u) | (install ? (uint32_t)VK_DIFF_INSTALL : 0u);
        for (int c = 0; c < 3; c++) req.spacing[c] = spacing ? spacing[c] : 1u;
        vk_diffusion_result res{};
        check(ctx_, vk_steady_diffusion(ctx_, &req, box, c_out, dense_out, &res));
        return res;
    }
    // What the header derives from a result, in double.  extent: the box's extents x, y, z (the volume's dimensions without a box).
    struct DiffusionValues { double flux, flux_in, flux_out, flux_mismatch, porosity, effective_diffusivity, tortuosity_factor, mean_concentration; };
    static DiffusionValues diffusion_values(const vk_diffusion_result &r, uint32_t axis, const uint32_t extent[3]) {
        DiffusionValues d{};
        const double fi = (double)r.Fin_q, fo = (double)r.Fout_q, mean = 0.5 * (fi + fo);
        d.flux_in = fi / 1073741824.0; d.flux_out = fo / 1073741824.0; d.flux = (fi + fo) / 2147483648.0;
        d.flux_mismatch = mean != 0.0 ? std::fabs(fi - fo) / std::fabs(mean) : (fi != fo ? INFINITY : 0.0);
        d.porosity = r.n_box ? (double)r.n_foreground / (double)r.n_box : 0.0;
        const double cross = (double)extent[(axis + 1u) % 3u] * (double)extent[(axis + 2u) % 3u];
        d.effective_diffusivity = cross > 0.0 ? d.flux * (double)extent[axis] / cross : 0.0;
        d.tortuosity_factor = d.effective_diffusivity > 0.0 ? d.porosity / d.effective_diffusivity : INFINITY;
        d.mean_concentration = r.n_foreground ? (double)r.sum_c_q / (1073741824.0 * (double)r.n_foreground) : 0.0;
        return d;
    }
    // sum_j links[j] sqrt(sum_c (spacing[c] d_c)^2) over the 13 offsets above the centre: the centre-line length in the units of the spacing (nullptr: 1 1 1).
    // Every adjacent pair counts, so the sum over-counts inside junction clumps.
    static double skeleton_length(const vk_skeleton_result &r, const uint32_t *spacing = nullptr) {
        double sum = 0.0;
        for (int j = 0; j < VK_SKEL_LINKS; j++) {
            const int o = 14 + j, d[3] = {o % 3 - 1, o / 3 % 3 - 1, o / 9 - 1};
            double q = 0.0;
            for (int c = 0; c < 3; c++) { const double e = (spacing ? (double)spacing[c] : 1.0) * d[c]; q += e * e; }
            sum += (double)r.links[j] * std::sqrt(q);
        }
        return sum;
    }
    // Frames in flight: the reference's queue runs ahead of the GPU (src/lib.rs:178-194), bounded by the swapchain
    // (get_current_texture, src/context.rs:252).  k surfaces, each on a stream of its own; 1 = one surface (the default).
    void frames_in_flight(uint32_t k) { check(ctx_, vk_ctx_frames_in_flight(ctx_, k)); }
    uint64_t frame_begin() { uint64_t id = 0; check(ctx_, vk_frame_begin(ctx_, &id)); return id; }  // the acquire
    void frame_end() { check(ctx_, vk_frame_end(ctx_)); }                                          // submit + present
    void frame_wait(uint64_t id) { check(ctx_, vk_frame_wait(ctx_, id)); }
    std::pair<std::vector<uint8_t>, ImageDimentions> capture_frame_of(uint64_t id) {
        ImageDimentions dims(width, height, 256);
        std::vector<uint8_t> out(dims.linear_size(), 0);
        check(ctx_, vk_frame_capture(ctx_, id, out.data(), out.size(), nullptr, nullptr, nullptr));
        return {out, dims};
    }
    void capture_frame_into(uint64_t id, std::vector<uint8_t> &out) {  // (the recorder's reused buffer)
        ImageDimentions dims(width, height, 256);
        if (out.size() != dims.linear_size()) out.assign(dims.linear_size(), 0);
        check(ctx_, vk_frame_capture(ctx_, id, out.data(), out.size(), nullptr, nullptr, nullptr));
    }
    std::string get_info() const {
        char name[256]; int cus = 0, is950 = 0; size_t mem = 0;
        check(ctx_, vk_device_info(ctx_, name, sizeof name, &cus, &is950, &mem));
        return std::string("Device name: ") + name + "\nBackend: HIP\nCompute units: " + std::to_string(cus) +
               "\nScreen format: " + (render_backbuffer.format == VK_OUT_RGBA16F ? "Rgba16Float" : "Rgba32Float");
    }
    // Context::render (context.rs:251-297): the present pass -- backbuffer -> ACES + sRGB -> Rgba8 at the
    // window size.  There is no surface to present to on a compute node.
    void render() {
        if (pass_presented) { pass_presented = false; return; }  // (the raycast pass has written the presented image itself)
        check(ctx_, vk_present(ctx_, width, height, 0));
    }
    uint32_t pass_flags(uint32_t flags) {  // what RaycastPipeline adds to a pass's flags under fuse_present
        if (fuse_present && width == render_backbuffer.width && height == render_backbuffer.height && !(flags & VK_RENDER_COUNT)) { pass_presented = true; return flags | VK_RENDER_PRESENT; }
        return flags;
    }
    // capture_frame (context.rs:299-302, screenshot.rs:37-77): the presented Rgba8 frame, rows padded to 256 B
    std::pair<std::vector<uint8_t>, ImageDimentions> capture_frame() {
        ImageDimentions dims(width, height, 256);
        std::vector<uint8_t> out(dims.linear_size(), 0);
        check(ctx_, vk_capture_frame(ctx_, out.data(), out.size(), nullptr, nullptr, nullptr));
        return {out, dims};
    }
    std::vector<float> read_backbuffer_f32() {
        const HdrBackBuffer &bb = render_backbuffer;
        size_t n = (size_t)bb.width * bb.height * 4;
        std::vector<float> out(n);
        if (bb.format == VK_OUT_RGBA32F) {
            check(ctx_, vk_readback(ctx_, out.data(), (size_t)bb.width * 16));
        } else {
            std::vector<uint16_t> h(n);
            check(ctx_, vk_readback(ctx_, h.data(), (size_t)bb.width * 8));
            for (size_t i = 0; i < n; i++) out[i] = half_to_float(h[i]);
        }
        return out;
    }
    static float half_to_float(uint16_t h) {
        uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu, b;
        if (e == 0) { if (!m) b = s; else { int k = -1; do { m <<= 1; k++; } while (!(m & 0x400u)); b = s | ((uint32_t)(112 - k) << 23) | ((m & 0x3ffu) << 13); } }
        else if (e == 31) b = s | 0x7f800000u | (m << 13);
        else b = s | ((e + 112) << 23) | (m << 13);
        float f; std::memcpy(&f, &b, 4); return f;
    }

  private:
    vk_ctx *ctx_ = nullptr;
    std::chrono::steady_clock::time_point timeline_;
    bool first_frame_ = true;
};

// src/context/volume_texture.rs:32-89
class VolumeTexture {
  public:
    uint32_t nx, ny, nz;
    int format;
    // dense x-fastest voxels (index x + nx*(y + ny*z))
    VolumeTexture(Context &ctx, const void *data, uint32_t nx_, uint32_t ny_, uint32_t nz_, int fmt = VK_FMT_R8_UNORM,
                  int layout = VK_LAYOUT_AUTO, const void *data2 = nullptr) : nx(nx_), ny(ny_), nz(nz_), format(fmt) {
        check(ctx.handle(), vk_volume_upload(ctx.handle(), data, data2, nx, ny, nz, fmt, layout));
    }
    // drop-in for the reference's include_bytes!("bonsai_256x256x256_uint8.raw") (absent from the checkout); fmt = VK_FMT_R16_UNORM: a raw
    // file of native-endian 16-bit integers (CT / MR data)
    static VolumeTexture from_raw(Context &ctx, const std::string &path, uint32_t nx = 256, uint32_t ny = 256, uint32_t nz = 256, int fmt = VK_FMT_R8_UNORM) {
        std::vector<char> buf = read_raw(path, nx, ny, nz, fmt);
        return VolumeTexture(ctx, buf.data(), nx, ny, nz, fmt);
    }
    // the bytes of such a file: nx * ny * nz voxels of 1 (R8_UNORM) or 2 (R16_UNORM) bytes.  An R16_UNORM file must have exactly that size (a
    // wrong --dims would otherwise show a sheared volume); an R8_UNORM file may be longer, as it always could: its leading bytes are taken
    static std::vector<char> read_raw(const std::string &path, uint32_t nx, uint32_t ny, uint32_t nz, int fmt) {
        if (fmt != VK_FMT_R8_UNORM && fmt != VK_FMT_R16_UNORM) throw std::runtime_error("raw volumes are R8_UNORM or R16_UNORM");
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        if (!f) throw std::runtime_error("cannot open " + path);
        std::vector<char> buf((size_t)nx * ny * nz * (fmt == VK_FMT_R16_UNORM ? 2 : 1));
        if (fmt == VK_FMT_R16_UNORM && (size_t)f.tellg() != buf.size()) throw std::runtime_error(path + ": expected " + std::to_string(buf.size()) + " bytes");
        f.seekg(0);
        f.read(buf.data(), (std::streamsize)buf.size());
        if ((size_t)f.gcount() != buf.size()) throw std::runtime_error(path + ": expected " + std::to_string(buf.size()) + " bytes");
        return buf;
    }
    static VolumeTexture generate(Context &ctx, int kind, uint32_t nx, uint32_t ny, uint32_t nz, int fmt = VK_FMT_R8_UNORM,
                                  uint32_t seed = 0x5EED0001u, uint32_t lo = 20, uint32_t span = 12, int layout = VK_LAYOUT_AUTO) {
        check(ctx.handle(), vk_volume_generate(ctx.handle(), kind, nx, ny, nz, fmt, seed, lo, span, layout));
        return VolumeTexture(nx, ny, nz, fmt);
    }

    // XorCompute::new + record (examples/xor/xor_compute.rs): density + normals from shaders/xor.wgsl
    static VolumeTexture generate_xor(Context &ctx, uint32_t nx = 256, uint32_t ny = 256, uint32_t nz = 256, float time = 0.f) {
        check(ctx.handle(), vk_volume_generate_xor(ctx.handle(), nx, ny, nz, time));
        return VolumeTexture(nx, ny, nz, VK_FMT_RGBA16F_PAIR);
    }

  private:
    VolumeTexture(uint32_t a, uint32_t b, uint32_t c, int f) : nx(a), ny(b), nz(c), format(f) {}
};

// examples/bonsai/raycast.rs (render pipeline) / examples/xor/raycast.rs (compute single + tile)
struct RaycastPipeline {
    int mode = VK_MODE_NAIVE_TRILINEAR;
    float dt_scale = 1.0f;
    uint32_t flags = 0;
    void record(Context &ctx) const {
        const HdrBackBuffer &bb = ctx.render_backbuffer;
        check(ctx.handle(), vk_render(ctx.handle(), mode, 0, 0, bb.width, bb.height, dt_scale, ctx.pass_flags(flags)));
    }
    void record_tile(Context &ctx, int32_t x, int32_t y, uint32_t w, uint32_t h) const {
        check(ctx.handle(), vk_render(ctx.handle(), mode, x, y, w, h, dt_scale, ctx.pass_flags(flags)));
    }
};

// trait Demo (src/lib.rs:37-43).  `init` is the static constructor D::init(Context&).
struct Demo {
    virtual ~Demo() = default;
    virtual void update(Context &) {}
    virtual void render(Context &) {}
};

// run::<D> (src/lib.rs:45-208) without the window: Context::update -> Demo::update -> Demo::render.
// in_flight > 1: the loop runs up to that many frames ahead of the GPU, every frame on a surface of its own.
// on_frame(ctx, id), if given, runs after each frame has been submitted -- the place of the reference's recorder
// (`if recording_status { context.capture_frame() ... }`, src/lib.rs:196-199), which with frames in flight captures a frame a few ids back.
struct NoFrameHook { void operator()(Context &, uint64_t) const {} };
template <class D, class OnFrame = NoFrameHook>
std::unique_ptr<D> run_headless(Context &ctx, uint32_t frames, double *mean_frame_ms = nullptr, uint32_t in_flight = 1, OnFrame on_frame = OnFrame()) {
    FrameCounter fc;
    if (in_flight > 1) ctx.frames_in_flight(in_flight);
    std::unique_ptr<D> demo = D::init(ctx);
    ctx.sync();  // (volume set-up is not frame time)
    auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < frames; i++) {
        ctx.update(fc);
        demo->update(ctx);
        fc.record();
        const uint64_t id = ctx.frame_begin();
        demo->render(ctx);
        ctx.render();  // src/lib.rs:178-182: demo.render, then context.render (present)
        ctx.frame_end();
        on_frame(ctx, id);
    }
    ctx.sync();
    if (mean_frame_ms) *mean_frame_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (frames ? frames : 1);
    return demo;
}

}  // namespace vokselis
