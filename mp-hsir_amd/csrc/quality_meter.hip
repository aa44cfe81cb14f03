// Quality meter: the per-band outputs of mphsir_quality for one scored batch become per-image values and are added to one row of a
// float64 table of running sums (include/mphsir.h holds the row layout and the per-image rule; mp-hsir_amd/validate.py is the user).
//
//   quality_meter_kernel   ONE workgroup of QM_NT threads.  Images are taken in chunks of QM_NT: thread i of a chunk walks the C bands
//                          of image b0 + i in ascending order (sum of the used bands' psnr and ssim, their number), divides once and
//                          leaves {psnr mean, ssim mean, sam, class} in LDS; after a barrier thread 0 adds the chunk's images to the
//                          row, which it holds in registers, in ascending image order; it writes the row once, after the last chunk.
//
// The work is B * C values (a few thousand at most) and the result must not depend on how a set was cut into batches, so the image
// sum is one chain of dependent float64 adds by design: the launch is latency-bound (a few hundred adds), a grid would buy nothing
// and an order that depends on scheduling is not allowed.  The band walk of a thread strides by C doubles from its neighbour's: two
// loads per band from buffers of a few KiB, all independent of the adds.  No atomics, nothing read back: capturable.
//
// Bounds: image b < n <= B and band c < C index psnr / ssim / use at b * C + c < B * C, sam_deg at b < B; the row lies at
// row * 8 .. row * 8 + 7 with 0 <= row < rows (all verified by the host before the launch); LDS slots are indexed by threadIdx.x < QM_NT.
#include "mphsir_host.h"
#include "mphsir_planar.h"

// sums and one divide: nothing here may be fused or reassociated, the table is compared bitwise with a float64 restatement
#pragma clang fp contract(off)

namespace mphsir {

constexpr int QM_NT = 256;
enum { QM_SCORED = 0, QM_NONFINITE = 1, QM_SKIPPED = 2 };

struct QualityMeterDev {
    const double* psnr; const double* ssim; const double* sam; const uint8_t* use; double* row;
    int C, n, reset;
};

__global__ __launch_bounds__(QM_NT) void quality_meter_kernel(QualityMeterDev a) {
    __shared__ double sp[QM_NT], ss[QM_NT], sa[QM_NT];
    __shared__ int cls[QM_NT];
    const int t = threadIdx.x;
    const double inf = __builtin_huge_val();
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0, r5 = inf, r6 = -inf, r7 = 0.0;
    if (t == 0 && !a.reset) {
        r0 = a.row[0]; r1 = a.row[1]; r2 = a.row[2]; r3 = a.row[3];
        r4 = a.row[4]; r5 = a.row[5]; r6 = a.row[6]; r7 = a.row[7];
    }
    for (int b0 = 0; b0 < a.n; b0 += QM_NT) {
        const int b = b0 + t;
        if (b < a.n) {
            const double* p = a.psnr + (long)b * a.C;
            const double* s = a.ssim + (long)b * a.C;
            const uint8_t* u = a.use ? a.use + (long)b * a.C : nullptr;
            double ap = 0.0, as = 0.0;
            int cnt = 0;
            // every band is inside the buffers, so the loads do not wait for the mask: the compiler issues a group of them ahead of the
            // adds (behind a branch on the mask each load waited for the one before: 29 us with cold inputs at C = 100, 25 us this way).  An unused band is
            // loaded and dropped by the select, never added: its NaN or inf stays out of the sums.
#pragma unroll 8
            for (int c = 0; c < a.C; ++c) {
                const double pv = p[c], sv = s[c];
                const bool on = !u || u[c] != 0;
                ap = on ? ap + pv : ap;
                as = on ? as + sv : as;
                cnt += on ? 1 : 0;
            }
            const double sam = a.sam[b];
            int k = QM_SKIPPED;
            if (cnt > 0) {
                ap = ap / (double)cnt;
                as = as / (double)cnt;
                k = finite(ap) && finite(as) && finite(sam) ? QM_SCORED : QM_NONFINITE;
            }
            sp[t] = ap;
            ss[t] = as;
            sa[t] = sam;
            cls[t] = k;
        }
        __syncthreads();                        // the chunk's per-image values are in LDS
        if (t == 0) {
            const int m = a.n - b0 < QM_NT ? a.n - b0 : QM_NT;
            for (int i = 0; i < m; ++i) {
                const int k = cls[i];
                if (k == QM_SCORED) {
                    const double v = sp[i];
                    r0 += 1.0;
                    r1 += v;
                    r2 += ss[i];
                    r3 += sa[i];
                    r5 = v < r5 ? v : r5;
                    r6 = v > r6 ? v : r6;
                } else if (k == QM_NONFINITE) {
                    r4 += 1.0;
                } else {
                    r7 += 1.0;
                }
            }
        }
        __syncthreads();                        // thread 0 is done with the chunk before the next one overwrites it
    }
    if (t == 0) {
        a.row[0] = r0; a.row[1] = r1; a.row[2] = r2; a.row[3] = r3;
        a.row[4] = r4; a.row[5] = r5; a.row[6] = r6; a.row[7] = r7;
    }
}

}  // namespace mphsir

extern "C" int mphsir_quality_meter(const mphsir_quality_meter_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "quality_meter");
    MPHSIR_REQUIRE(a->psnr && a->ssim && a->sam_deg && a->sam_pixels && a->table, "quality_meter: null pointer");
    MPHSIR_REQUIRE(a->B >= 1 && a->C >= 1 && a->rows >= 1, "quality_meter: bad sizes (B %d, C %d, rows %d: each at least 1)", a->B, a->C, a->rows);
    MPHSIR_REQUIRE(a->n >= 0 && a->n <= a->B, "quality_meter: n %d outside [0, B = %d]", a->n, a->B);
    MPHSIR_REQUIRE(a->row >= 0 && a->row < a->rows, "quality_meter: row %d outside the table's %d rows", a->row, a->rows);
    MPHSIR_REQUIRE((reinterpret_cast<uintptr_t>(a->table) & 7) == 0 && (reinterpret_cast<uintptr_t>(a->psnr) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(a->ssim) & 7) == 0 && (reinterpret_cast<uintptr_t>(a->sam_deg) & 7) == 0,
                   "quality_meter: float64 pointers must be 8-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    QualityMeterDev d{a->psnr, a->ssim, a->sam_deg, a->use, a->table + (long)a->row * 8, a->C, a->n, a->reset};
    MPHSIR_LAUNCH(MPHSIR_K_QUALITY, quality_meter_kernel, dim3(1), dim3(QM_NT), 0, s, d);
    return MPHSIR_OK;
}
