// Training criterion (include/dfx_criterion.h): matching costs, set loss forward and backward for every prediction set of
// one criterion call in one launch each, and the host-side linear sum assignment.
//
// The work is tiny (a recipe has 6 to 9 sets of at most B * 300 rows of 3 + 4 floats) and the reference spends it in several
// hundred launches; here it is three.  Nothing is bandwidth- or ALU-bound at these sizes, so the kernels buy accuracy with
// the idle ALUs: the set loss and its gradients are evaluated in fp64 per element and rounded once on store (every stored
// value is the fp32 nearest to the exact one up to the fp64 evaluation error), and every sum runs in double in an order
// fixed by the shapes alone - per-thread strided partials, an xor butterfly per wave, the waves in index order.  No atomics.
#include "dfx_common.h"
#include "dfx_criterion.h"

#include <math.h>
#include <cmath>

#include <algorithm>
#include <limits>

namespace {

using dfx::fail;

constexpr int kLossThreads = 512;       // one workgroup per set: 8 waves walk the set's B * Q rows (1024 threads cap the
                                        // kernel at 128 VGPRs, which its fp64 arithmetic overflows into scratch)
constexpr int kMaxSets = 64;
constexpr int kMaxImages = 4096;

// ---- shared arithmetic ------------------------------------------------------------------------------------------
// GIoU of two (cx, cy, w, h) boxes, in T (float for the costs, double for the loss)
template <typename T>
__device__ __forceinline__ T giou_cxcywh(const T *a, const T *b)
{
    const T ax0 = a[0] - T(0.5) * a[2], ay0 = a[1] - T(0.5) * a[3], ax1 = a[0] + T(0.5) * a[2], ay1 = a[1] + T(0.5) * a[3];
    const T bx0 = b[0] - T(0.5) * b[2], by0 = b[1] - T(0.5) * b[3], bx1 = b[0] + T(0.5) * b[2], by1 = b[1] + T(0.5) * b[3];
    const T area_a = (ax1 - ax0) * (ay1 - ay0), area_b = (bx1 - bx0) * (by1 - by0);
    const T iw = fmax(fmin(ax1, bx1) - fmax(ax0, bx0), T(0)), ih = fmax(fmin(ay1, by1) - fmax(ay0, by0), T(0));
    const T inter = iw * ih, uni = area_a + area_b - inter;
    const T ew = fmax(fmax(ax1, bx1) - fmin(ax0, bx0), T(0)), eh = fmax(fmax(ay1, by1) - fmin(ay0, by0), T(0));
    const T enc = ew * eh;
    return inter / uni - (enc - uni) / enc;
}

// set that owns `row`: the last s whose first row is <= row (the prefixes grow with s)
__device__ __forceinline__ int set_of_row(const int *desc, int S, int row)
{
    int s = 0;
    while (s + 1 < S && row >= desc[3 * (s + 1) + 1]) ++s;
    return s;
}

// label of a row: 0..2, or 3 = no column (unmatched, or a stored label outside 0..2)
__device__ __forceinline__ int row_label(const int *tgt_labels, int g, int Ttot, int zero_labels)
{
    if (g < 0 || g >= Ttot) return 3;
    if (zero_labels) return 0;
    const int l = tgt_labels[g];
    return l >= 0 && l < 3 ? l : 3;
}

__device__ __forceinline__ int argmax3(float x0, float x1, float x2)
{
    int am = 0;
    float top = x0;
    if (x1 > top) { am = 1; top = x1; }
    if (x2 > top) am = 2;
    return am;
}

// alpha-free focal term of one logit: BCE(x, t) * (1 - p_t)^2 and its derivative in x
__device__ __forceinline__ double focal(double x, bool t)
{
    const double e = exp(-fabs(x));
    const double ce = fmax(x, 0.0) - (t ? x : 0.0) + log1p(e);
    const double p = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    const double m = t ? 1.0 - p : p;           // 1 - p_t
    return ce * m * m;
}

__device__ __forceinline__ double focal_grad(double x, bool t)
{
    const double e = exp(-fabs(x));
    const double ce = fmax(x, 0.0) - (t ? x : 0.0) + log1p(e);
    const double p = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    const double q = x >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);      // 1 - p without cancellation
    const double m = t ? q : p;
    const double dce = t ? -q : p;              // p - t
    const double dm = t ? -p * q : p * q;
    return dce * m * m + 2.0 * ce * m * dm;
}

// ---- matching costs ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void match_cost_kernel(const float *__restrict__ logits, const float *__restrict__ boxes,
                                                         const int *__restrict__ tgt_labels, const float *__restrict__ tgt_boxes,
                                                         const int *__restrict__ desc, int S, int B, int Ttot, long total,
                                                         float w_class, float w_bbox, float w_giou, float *__restrict__ cost)
{
    const int *off = desc + 3 * S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long rem = i;
        int s = 0;
        for (; s + 1 < S; ++s) {
            const long block = (long)Ttot * desc[3 * s];
            if (rem < block) break;
            rem -= block;
        }
        const int Q = desc[3 * s], row0 = desc[3 * s + 1], zero_labels = desc[3 * s + 2];
        int b = 0;
        while (b + 1 < B && rem >= (long)Q * off[b + 1]) ++b;
        const int t0 = off[b], T = off[b + 1] - t0;
        if (T <= 0) continue;                                   // (a descriptor that does not describe `total` pairs)
        rem -= (long)Q * t0;
        const int q = (int)(rem / T), t = (int)(rem - (long)q * T);
        if (rem < 0 || q >= Q) continue;
        const long row = (long)row0 + (long)b * Q + q;
        const int g = t0 + t;
        const int label = row_label(tgt_labels, g, Ttot, zero_labels);
        float c = std::numeric_limits<float>::quiet_NaN();
        if (label < 3) {
            const float p = 1.0f / (1.0f + expf(-logits[row * 3 + label]));
            const float neg = 0.75f * (p * p) * (-logf(1.0f - p + 1e-8f));
            const float pos = 0.25f * ((1.0f - p) * (1.0f - p)) * (-logf(p + 1e-8f));
            float a[4], tb[4], l1 = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[k] = boxes[row * 4 + k];
                tb[k] = tgt_boxes[(long)g * 4 + k];
                l1 += fabsf(a[k] - tb[k]);
            }
            c = w_bbox * l1 + w_class * (pos - neg) + w_giou * (-giou_cxcywh<float>(a, tb));
        }
        cost[i] = c;
    }
}

// ---- set loss, forward -------------------------------------------------------------------------------------------
// sum over the workgroup in a fixed order; every thread gets the result.  `slot` holds one double per wave.
__device__ __forceinline__ double block_sum(double v, double *slot)
{
    v = dfx::wave_sum(v);
    __syncthreads();                                            // the slots may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < kLossThreads / 64; ++w) total += slot[w];
    return total;
}

__global__ __launch_bounds__(kLossThreads) void set_loss_forward_kernel(
    const float *__restrict__ logits, const float *__restrict__ boxes, const int *__restrict__ tgt_labels,
    const float *__restrict__ tgt_boxes, const int *__restrict__ row_target, const int *__restrict__ desc, int S, int B, int Ttot,
    double inv_num_boxes, float *__restrict__ out)
{
    __shared__ double slot[kLossThreads / 64];
    const int s = blockIdx.x;
    const int Q = desc[3 * s], row0 = desc[3 * s + 1], zero_labels = desc[3 * s + 2];
    const int *off = desc + 3 * S;
    const double alpha2 = (double)0.001f;                       // the reference's alpha table is fp32
    double ce = 0.0, l1 = 0.0, gl = 0.0, matched = 0.0, correct = 0.0, card = 0.0;
    for (int b = 0; b < B; ++b) {
        double objects = 0.0;
        for (int q = threadIdx.x; q < Q; q += kLossThreads) {
            const long row = (long)row0 + (long)b * Q + q;
            const float x0 = logits[row * 3], x1 = logits[row * 3 + 1], x2 = logits[row * 3 + 2];
            const int g = row_target[row];
            const int label = row_label(tgt_labels, g, Ttot, zero_labels);
            const int am = argmax3(x0, x1, x2);
            objects += am != 2;
            ce += focal((double)x1, label == 1) + alpha2 * focal((double)x2, label != 1);
            if (g >= 0 && g < Ttot) {
                matched += 1.0;
                correct += am == label;
                double a[4], tb[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = (double)boxes[row * 4 + k];
                    tb[k] = (double)tgt_boxes[(long)g * 4 + k];
                    l1 += fabs(a[k] - tb[k]);
                }
                gl += 1.0 - giou_cxcywh<double>(a, tb);
            }
        }
        objects = block_sum(objects, slot);
        card += fabs(objects - (double)(off[b + 1] - off[b]));
    }
    ce = block_sum(ce, slot);
    l1 = block_sum(l1, slot);
    gl = block_sum(gl, slot);
    matched = block_sum(matched, slot);
    correct = block_sum(correct, slot);
    if (threadIdx.x == 0) {
        float *o = out + 5 * s;
        o[0] = (float)(ce * inv_num_boxes);
        o[1] = (float)(matched > 0.0 ? 100.0 - correct * 100.0 / matched : 100.0);
        o[2] = (float)(l1 * inv_num_boxes);
        o[3] = (float)(gl * inv_num_boxes);
        o[4] = (float)(B > 0 ? card / B : 0.0);
    }
}

// ---- set loss, backward ------------------------------------------------------------------------------------------
// d(1 - GIoU)/d(cx, cy, w, h) of box a against b, times `scale`, by hand in reverse mode
__device__ __forceinline__ void giou_loss_grad(const double *a, const double *b, double scale, double *grad)
{
    double lo[2], hi[2], blo[2], bhi[2], iw[2], ew[2];
    bool overlap[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        lo[d] = a[d] - 0.5 * a[2 + d];
        hi[d] = a[d] + 0.5 * a[2 + d];
        blo[d] = b[d] - 0.5 * b[2 + d];
        bhi[d] = b[d] + 0.5 * b[2 + d];
        const double raw = fmin(hi[d], bhi[d]) - fmax(lo[d], blo[d]);
        // the clamp at 0 passes the gradient AT 0 as well, as the reference's clamp(min=0) does: a prediction of zero width
        // between the target's edges has raw == 0, and the intersection grows with its width at the rate of the other side
        overlap[d] = raw >= 0.0;
        iw[d] = fmax(raw, 0.0);
        ew[d] = fmax(fmax(hi[d], bhi[d]) - fmin(lo[d], blo[d]), 0.0);
    }
    const double side[2] = {hi[0] - lo[0], hi[1] - lo[1]};
    const double area_a = side[0] * side[1], area_b = (bhi[0] - blo[0]) * (bhi[1] - blo[1]);
    const double inter = iw[0] * iw[1], uni = area_a + area_b - inter, enc = ew[0] * ew[1];
    // giou = inter / uni - 1 + uni / enc;  loss = 1 - giou
    const double g_giou = -scale;
    const double g_enc = -g_giou * uni / (enc * enc);
    const double g_uni = g_giou / enc - g_giou * inter / (uni * uni);
    const double g_inter = g_giou / uni - g_uni;
    const double g_area = g_uni;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int o = 1 - d;
        double g_lo = -g_area * side[o], g_hi = g_area * side[o];
        const double g_iw = overlap[d] ? g_inter * iw[o] : 0.0;            // through the clamp at 0
        if (lo[d] > blo[d]) g_lo -= g_iw;                                  // max(lo, blo)
        if (hi[d] < bhi[d]) g_hi += g_iw;                                  // min(hi, bhi)
        const double g_ew = ew[d] > 0.0 ? g_enc * ew[o] : 0.0;
        if (lo[d] < blo[d]) g_lo -= g_ew;                                  // min(lo, blo)
        if (hi[d] > bhi[d]) g_hi += g_ew;                                  // max(hi, bhi)
        grad[d] = g_lo + g_hi;
        grad[2 + d] = 0.5 * (g_hi - g_lo);
    }
}

__global__ __launch_bounds__(256) void set_loss_backward_kernel(
    const float *__restrict__ grad_out, const float *__restrict__ logits, const float *__restrict__ boxes,
    const int *__restrict__ tgt_labels, const float *__restrict__ tgt_boxes, const int *__restrict__ row_target,
    const int *__restrict__ desc, int S, int rows, int Ttot, double inv_num_boxes, float *__restrict__ grad_logits,
    float *__restrict__ grad_boxes)
{
    for (long row = (long)blockIdx.x * 256 + threadIdx.x; row < rows; row += (long)gridDim.x * 256) {
        const int s = set_of_row(desc, S, (int)row);
        const int g = row_target[row];
        const bool is_matched = g >= 0 && g < Ttot;
        if (grad_logits) {
            const int label = row_label(tgt_labels, g, Ttot, desc[3 * s + 2]);
            const double go = (double)grad_out[5 * s] * inv_num_boxes;
            grad_logits[row * 3] = 0.0f;
            grad_logits[row * 3 + 1] = (float)(go * focal_grad((double)logits[row * 3 + 1], label == 1));
            grad_logits[row * 3 + 2] = (float)(go * (double)0.001f * focal_grad((double)logits[row * 3 + 2], label != 1));
        }
        if (grad_boxes) {
            double gb[4] = {0.0, 0.0, 0.0, 0.0};
            if (is_matched) {
                const double go_l1 = (double)grad_out[5 * s + 2] * inv_num_boxes;
                const double go_giou = (double)grad_out[5 * s + 3] * inv_num_boxes;
                double a[4], tb[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = (double)boxes[row * 4 + k];
                    tb[k] = (double)tgt_boxes[(long)g * 4 + k];
                }
                giou_loss_grad(a, tb, go_giou, gb);
#pragma unroll
                for (int k = 0; k < 4; ++k) gb[k] += a[k] > tb[k] ? go_l1 : a[k] < tb[k] ? -go_l1 : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) grad_boxes[row * 4 + k] = is_matched ? (float)gb[k] : 0.0f;
        }
    }
}

// ---- argument checks ---------------------------------------------------------------------------------------------
// <0: error, 1: nothing to do, 0: go
int check_layout(const char *what, int S, int B, int rows, int Ttot)
{
    if (S < 0 || B < 0 || rows < 0 || Ttot < 0) return fail(DFX_EINVAL, "%s: bad dimension (S=%d B=%d rows=%d Ttot=%d)", what, S, B, rows, Ttot);
    if (S > kMaxSets || B > kMaxImages) return fail(DFX_ERANGE, "%s: at most %d sets and %d images", what, kMaxSets, kMaxImages);
    if ((long)rows * 4 >= (1L << 31)) return fail(DFX_ERANGE, "%s: too many rows", what);
    return S == 0 || B == 0 || rows == 0 ? 1 : 0;
}

// ---- linear sum assignment (host) ----------------------------------------------------------------------------------
// Shortest augmenting paths with dual variables (D. F. Crouse, "On implementing 2D rectangular assignment algorithms",
// IEEE TAES 52(4), 2016) on an nr x nc problem with nr <= nc; cost(i, j) reads the caller's matrix either way round.
template <typename Cost>
bool lsap_rows_le_cols(int nr, int nc, Cost cost, std::vector<int> &col4row)
{
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> u(nr, 0.0), v(nc, 0.0), shortest(nc);
    std::vector<int> path(nc, -1), row4col(nc, -1), remaining(nc);
    std::vector<char> in_sr(nr), in_sc(nc);
    col4row.assign(nr, -1);
    for (int cur = 0; cur < nr; ++cur) {
        double min_val = 0.0;
        int left = nc, sink = -1, i = cur;
        for (int it = 0; it < nc; ++it) remaining[it] = nc - it - 1;      // reversed: ties go to the lower column
        std::fill(in_sr.begin(), in_sr.end(), 0);
        std::fill(in_sc.begin(), in_sc.end(), 0);
        std::fill(shortest.begin(), shortest.end(), inf);
        while (sink < 0) {
            int index = -1;
            double lowest = inf;
            in_sr[i] = 1;
            for (int it = 0; it < left; ++it) {
                const int j = remaining[it];
                const double r = min_val + cost(i, j) - u[i] - v[j];
                if (r < shortest[j]) {
                    path[j] = i;
                    shortest[j] = r;
                }
                if (shortest[j] < lowest || (shortest[j] == lowest && row4col[j] < 0)) {
                    lowest = shortest[j];
                    index = it;
                }
            }
            min_val = lowest;
            if (index < 0 || min_val == inf) return false;
            const int j = remaining[index];
            if (row4col[j] < 0) sink = j;
            else i = row4col[j];
            in_sc[j] = 1;
            remaining[index] = remaining[--left];
        }
        u[cur] += min_val;
        for (int r = 0; r < nr; ++r)
            if (in_sr[r] && r != cur) u[r] += min_val - shortest[col4row[r]];
        for (int j = 0; j < nc; ++j)
            if (in_sc[j]) v[j] -= min_val - shortest[j];
        for (int j = sink;;) {
            const int r = path[j];
            row4col[j] = r;
            std::swap(col4row[r], j);
            if (r == cur) break;
        }
    }
    return true;
}

// one [Q, T] block -> pairs sorted by row; returns 0 or a negative code
int lsap_block(const float *cost, int Q, int T, int *rows, int *cols)
{
    if (Q == 0 || T == 0) return DFX_OK;
    for (long i = 0; i < (long)Q * T; ++i)
        if (!std::isfinite(cost[i])) return fail(DFX_ENONFINITE, "lsap: cost matrix contains a NaN or an infinity");
    std::vector<int> match;
    bool ok;
    if (Q <= T) {
        ok = lsap_rows_le_cols(Q, T, [&](int i, int j) { return (double)cost[(long)i * T + j]; }, match);
        for (int i = 0; ok && i < Q; ++i) { rows[i] = i; cols[i] = match[i]; }
    } else {
        ok = lsap_rows_le_cols(T, Q, [&](int i, int j) { return (double)cost[(long)j * T + i]; }, match);   // the transpose
        if (ok) {
            std::vector<int> order(T);
            for (int t = 0; t < T; ++t) order[t] = t;
            std::sort(order.begin(), order.end(), [&](int x, int y) { return match[x] < match[y]; });
            for (int k = 0; k < T; ++k) { rows[k] = match[order[k]]; cols[k] = order[k]; }
        }
    }
    return ok ? DFX_OK : fail(DFX_EINVAL, "lsap: cost matrix is infeasible");
}

}  // namespace

extern "C" int dfx_match_cost_f32(const float *logits, const float *boxes, const int *tgt_labels, const float *tgt_boxes,
                                  const int *desc, int S, int B, int rows, int Ttot, float cost_class, float cost_bbox,
                                  float cost_giou, float *cost, void *stream)
{
    const int rc = check_layout("match_cost", S, B, rows, Ttot);
    if (rc < 0) return rc;
    if (rc == 1 || Ttot == 0) return DFX_OK;
    if (rows % B) return fail(DFX_EINVAL, "match_cost: rows must be B * sum(Q)");
    const long total = (long)(rows / B) * Ttot;
    if (total >= (1L << 31)) return fail(DFX_ERANGE, "match_cost: cost buffer exceeds 2^31 elements");
    if (!logits || !boxes || !tgt_labels || !tgt_boxes || !desc || !cost) return fail(DFX_EINVAL, "match_cost: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(match_cost_kernel, dim3(dfx::grid_for(total)), dim3(256), 0, st, logits, boxes, tgt_labels, tgt_boxes, desc,
                       S, B, Ttot, total, cost_class, cost_bbox, cost_giou, cost);
    return dfx::check_launch("match_cost");
}

extern "C" int dfx_set_loss_forward_f32(const float *logits, const float *boxes, const int *tgt_labels, const float *tgt_boxes,
                                        const int *row_target, const int *desc, int S, int B, int rows, int Ttot,
                                        double inv_num_boxes, float *out, void *stream)
{
    const int rc = check_layout("set_loss_forward", S, B, rows, Ttot);
    if (rc < 0) return rc;
    if (S == 0) return DFX_OK;
    if (!out || !desc) return fail(DFX_EINVAL, "set_loss_forward: null pointer");
    if (rows > 0 && (!logits || !boxes || !row_target)) return fail(DFX_EINVAL, "set_loss_forward: null pointer");
    if (Ttot > 0 && (!tgt_labels || !tgt_boxes)) return fail(DFX_EINVAL, "set_loss_forward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(set_loss_forward_kernel, dim3(S), dim3(kLossThreads), 0, st, logits, boxes, tgt_labels, tgt_boxes,
                       row_target, desc, S, B, Ttot, inv_num_boxes, out);
    return dfx::check_launch("set_loss_forward");
}

extern "C" int dfx_set_loss_backward_f32(const float *grad_out, const float *logits, const float *boxes, const int *tgt_labels,
                                         const float *tgt_boxes, const int *row_target, const int *desc, int S, int B, int rows,
                                         int Ttot, double inv_num_boxes, float *grad_logits, float *grad_boxes, void *stream)
{
    const int rc = check_layout("set_loss_backward", S, B, rows, Ttot);
    if (rc < 0) return rc;
    if (rc == 1 || (!grad_logits && !grad_boxes)) return DFX_OK;
    if (!grad_out || !logits || !boxes || !row_target || !desc) return fail(DFX_EINVAL, "set_loss_backward: null pointer");
    if (Ttot > 0 && (!tgt_labels || !tgt_boxes)) return fail(DFX_EINVAL, "set_loss_backward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(set_loss_backward_kernel, dim3(dfx::grid_for(rows)), dim3(256), 0, st, grad_out, logits, boxes, tgt_labels,
                       tgt_boxes, row_target, desc, S, rows, Ttot, inv_num_boxes, grad_logits, grad_boxes);
    return dfx::check_launch("set_loss_backward");
}

extern "C" int dfx_lsap_f32(const float *cost, int Q, int T, int *rows, int *cols)
{
    if (Q < 0 || T < 0) return fail(DFX_EINVAL, "lsap: bad dimension (Q=%d T=%d)", Q, T);
    if (Q == 0 || T == 0) return DFX_OK;
    if (!cost || !rows || !cols) return fail(DFX_EINVAL, "lsap: null pointer");
    return lsap_block(cost, Q, T, rows, cols);
}

extern "C" int dfx_lsap_ragged_f32(const float *cost, const int *desc, int S, int B, int rows, int Ttot, int *row_target)
{
    const int rc = check_layout("lsap_ragged", S, B, rows, Ttot);
    if (rc < 0) return rc;
    if (rows > 0 && !row_target) return fail(DFX_EINVAL, "lsap_ragged: null pointer");
    std::fill(row_target, row_target + rows, -1);
    if (rc == 1 || Ttot == 0) return DFX_OK;
    if (!cost || !desc) return fail(DFX_EINVAL, "lsap_ragged: null pointer");
    const int *off = desc + 3 * S;
    if (off[0] != 0 || off[B] != Ttot) return fail(DFX_EINVAL, "lsap_ragged: target offsets do not span 0 .. Ttot");
    std::vector<int> qi, ti;
    long base = 0, row_end = 0;
    for (int s = 0; s < S; ++s) {
        const int Q = desc[3 * s], row0 = desc[3 * s + 1];
        if (Q < 0 || row0 != row_end || (long)row0 + (long)B * Q > rows) return fail(DFX_EINVAL, "lsap_ragged: descriptor does not tile the rows");
        row_end = (long)row0 + (long)B * Q;
        for (int b = 0; b < B; ++b) {
            const int T = off[b + 1] - off[b];
            if (T < 0) return fail(DFX_EINVAL, "lsap_ragged: target offsets must not decrease");
            const int n = std::min(Q, T);
            qi.resize(n);
            ti.resize(n);
            const int err = lsap_block(cost + base + (long)Q * off[b], Q, T, qi.data(), ti.data());
            if (err) return err;
            for (int k = 0; k < n; ++k) row_target[row0 + b * Q + qi[k]] = off[b] + ti[k];
        }
        base += (long)Q * Ttot;
    }
    return DFX_OK;
}
