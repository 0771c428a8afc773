// pnp_host_check.cpp — the host pose solver (csrc/pnp_host.hip) as a stand-alone program, for runs under host sanitizers.
//
// Links pnp_host.hip alone (the error text of plan.hip is restated below) and runs every record of a file that
// tools/pnp_host_check.py wrote through esahrnet_pnp_batch_w_ex (and esahrnet_pnp_batch_ex where the record has keypoint
// rows), with 1 and 4 threads, with and without a report buffer.  It checks what tests/test_pose_report_host.py checks at the
// C level: the poses do not depend on the report or the thread count, nor do the report's bits, and the old entries are the
// new ones with a null report.  A second file holds candidate records for esahrnet_pnp_batch_cand: the same bits at 1 and 4
// threads, with and without a report, and with one candidate the bits of esahrnet_pnp_batch_ex.  The same candidates go through
// esahrnet_pnp_batch_cand_pts as records in image pixels (make_record: M candidates and one, count = 0 images, NaN slots), held to
// the bits of the entries on the rows, and every argument that entry refuses is tried.  Exit status 0 and "ok" when all of it
// holds.  Pure host code: no GPU is touched.
//
// Build and run (tools/pnp_host_check.py does both):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/pnp_host_check.cpp esa-pose-estimation_amd/csrc/pnp_host.hip -fsanitize=address,undefined -o pnp_host_check
//   ./pnp_host_check records.bin candidates.bin
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../include/esahrnet.h"
#include "../esa-pose-estimation_amd/csrc/correspond.h"

namespace esa {
static char g_err[512];
int set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}
}  // namespace esa

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return fread(v.data(), sizeof(T), n, f) == n;
}

static bool same(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

// The record esahrnet_correspondences_cand writes (include/esahrnet.h), made on the host from the first Mr of the M candidate rows
// with the functions of csrc/correspond.h: cpts [m][k][Mr][2], cw [m][k][Mr][3], cpeak [m][k][Mr], count [m], order [m][k], each
// exactly sized.  Every third image (i % 3 == 2) is an invalid crop: count 0, order -1, zeros.
static void make_record(const std::vector<float>& cand, const std::vector<double>& hess, int m, int k, int M, int Mr,
                        const std::vector<int32_t>& boxes, const std::vector<double>& rates, double thresh, int min_k, int mode,
                        std::vector<double>& cpts, std::vector<double>& cw, std::vector<float>& cpeak, std::vector<int32_t>& count,
                        std::vector<int32_t>& order) {
    cpts.assign((size_t)m * k * Mr * 2, 0.0);
    cw.assign((size_t)m * k * Mr * 3, 0.0);
    cpeak.assign((size_t)m * k * Mr, 0.f);
    count.assign(m, 0);
    order.assign((size_t)m * k, -1);
    for (int i = 0; i < m; ++i) {
        if (i % 3 == 2) continue;
        const float* c = &cand[(size_t)i * k * M * 3];
        int above = 0;
        for (int j = 0; j < k; ++j) above += (double)c[j * M * 3 + 2] > thresh;
        const int n = esa::corr_count(above, min_k, k);
        std::vector<int> ord(k);
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return esa::corr_before(c[a * M * 3 + 2], a, c[b * M * 3 + 2], b); });
        const double inv = esa::corr_inv_rate(rates[i]);
        for (int s = 0; s < n; ++s) {
            const int j = ord[s];
            order[(size_t)i * k + s] = j;
            for (int mm = 0; mm < Mr; ++mm) {
                const float* r = c + ((size_t)j * M + mm) * 3;
                const size_t at = ((size_t)i * k + s) * Mr + mm;
                cpeak[at] = r[2];
                if (std::isfinite(r[0]) && std::isfinite(r[1])) {
                    cpts[at * 2 + 0] = esa::corr_to_image(r[0], inv, boxes[i * 2]);
                    cpts[at * 2 + 1] = esa::corr_to_image(r[1], inv, boxes[i * 2 + 1]);
                    if (mode) esa::corr_hessian_weight(&hess[(((size_t)i * k + j) * M + mm) * 3], rates[i], &cw[at * 3]);
                    else cw[at * 3] = cw[at * 3 + 2] = (double)r[2];
                } else {
                    cpts[at * 2] = cpts[at * 2 + 1] = NAN;
                }
            }
        }
        count[i] = n;
    }
}

// candidate records: int32 (m, k, M), cand f32 [m][k][M][3], kp3d f64 [k][3], K9, boxes int32 [m][2], rates f64 [m],
// (thresh, min_k, min_ratio) f64.  Every buffer handed to the library has its exact size.
static int check_candidates(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); return 2; }
    int32_t head[3];
    int nrec = 0;
    const size_t R = ESAHRNET_POSE_REPORT_DOUBLES;
    while (std::fread(head, sizeof(int32_t), 3, f) == 3) {
        const int m = head[0], k = head[1], M = head[2];
        std::vector<float> cand;
        std::vector<double> kp3d, K9, rates, sel;
        std::vector<int32_t> boxes;
        if (!(read_vec(f, cand, (size_t)m * k * M * 3) && read_vec(f, kp3d, (size_t)k * 3) && read_vec(f, K9, 9) &&
              read_vec(f, boxes, (size_t)m * 2) && read_vec(f, rates, m) && read_vec(f, sel, 3))) {
            std::fprintf(stderr, "candidate record %d is cut short\n", nrec);
            return 2;
        }
        std::vector<double> q0, t0, rep0;
        std::vector<int32_t> used0;
        for (int threads : {1, 4})
            for (int with_report = 0; with_report < 2; ++with_report) {
                std::vector<double> q((size_t)m * 4), t((size_t)m * 3), rep(with_report ? m * R : 0);
                std::vector<int32_t> used((size_t)m * k);
                if (esahrnet_pnp_batch_cand(cand.data(), m, k, M, kp3d.data(), K9.data(), boxes.data(), rates.data(), sel[0], (int)sel[1],
                                            sel[2], threads, q.data(), t.data(), with_report ? rep.data() : nullptr, used.data())) {
                    std::fprintf(stderr, "candidate record %d: %s\n", nrec, esa::g_err);
                    return 1;
                }
                if (q0.empty()) { q0 = q; t0 = t; used0 = used; }
                if (with_report && rep0.empty()) rep0 = rep;
                if (!same(q, q0) || !same(t, t0) || used != used0 || (with_report && !same(rep, rep0))) {
                    std::fprintf(stderr, "candidate record %d: results differ (threads %d, report %d)\n", nrec, threads, with_report);
                    return 1;
                }
            }
        // candidate 0 alone, through both entries
        std::vector<float> first((size_t)m * k * 3);
        for (size_t i = 0; i < (size_t)m * k; ++i) std::memcpy(&first[i * 3], &cand[i * M * 3], 3 * sizeof(float));
        std::vector<double> q1((size_t)m * 4), t1((size_t)m * 3), rep1(m * R), q2((size_t)m * 4), t2((size_t)m * 3), rep2(m * R);
        std::vector<int32_t> used1((size_t)m * k);
        if (esahrnet_pnp_batch_cand(first.data(), m, k, 1, kp3d.data(), K9.data(), boxes.data(), rates.data(), sel[0], (int)sel[1], sel[2],
                                    4, q1.data(), t1.data(), rep1.data(), used1.data()) ||
            esahrnet_pnp_batch_ex(first.data(), m, k, kp3d.data(), K9.data(), boxes.data(), rates.data(), sel[0], (int)sel[1], 4,
                                  q2.data(), t2.data(), rep2.data())) {
            std::fprintf(stderr, "candidate record %d: %s\n", nrec, esa::g_err);
            return 1;
        }
        if (!same(q1, q2) || !same(t1, t2) || !same(rep1, rep2)) {
            std::fprintf(stderr, "candidate record %d: one candidate is not esahrnet_pnp_batch_ex\n", nrec);
            return 1;
        }
        // esahrnet_pnp_batch_cand_w: a Hessian per candidate row (NaN where the row is, a saddle every 13th), exactly sized;
        // the same bits at 1 and 4 threads, with and without a report; with hess null the bits of esahrnet_pnp_batch_cand
        std::vector<double> hess((size_t)m * k * M * 3), qw0, tw0, repw0;
        for (size_t i = 0; i < (size_t)m * k * M; ++i) {
            const bool none = std::isnan(cand[i * 3]);
            hess[i * 3 + 0] = none ? NAN : i % 13 == 12 ? 0.1 : -(0.05 + 0.01 * (double)(i % 7));
            hess[i * 3 + 1] = none ? NAN : 0.01 * ((double)(i % 5) - 2.0);
            hess[i * 3 + 2] = none ? NAN : -(0.08 + 0.01 * (double)(i % 3));
        }
        std::vector<int32_t> usedw0;
        for (int threads : {1, 4})
            for (int with_report = 0; with_report < 2; ++with_report)
                for (int with_hess = 0; with_hess < 2; ++with_hess) {
                    std::vector<double> q((size_t)m * 4), t((size_t)m * 3), rep(with_report ? m * R : 0);
                    std::vector<int32_t> used((size_t)m * k);
                    if (esahrnet_pnp_batch_cand_w(cand.data(), with_hess ? hess.data() : nullptr, m, k, M, kp3d.data(), K9.data(), boxes.data(),
                                                  rates.data(), sel[0], (int)sel[1], sel[2], threads, q.data(), t.data(),
                                                  with_report ? rep.data() : nullptr, used.data())) {
                        std::fprintf(stderr, "candidate record %d: %s\n", nrec, esa::g_err);
                        return 1;
                    }
                    if (with_hess && qw0.empty()) { qw0 = q; tw0 = t; usedw0 = used; }
                    if (with_hess && with_report && repw0.empty()) repw0 = rep;
                    const bool ok = with_hess ? same(q, qw0) && same(t, tw0) && used == usedw0 && (!with_report || same(rep, repw0))
                                              : same(q, q0) && same(t, t0) && used == used0 && (!with_report || same(rep, rep0));
                    if (!ok) {
                        std::fprintf(stderr, "candidate record %d: weighted results differ (threads %d, report %d, hess %d)\n", nrec, threads,
                                     with_report, with_hess);
                        return 1;
                    }
                }
        // esahrnet_pnp_batch_cand_pts on the record of these rows in image pixels (made here with csrc/correspond.h, as the device
        // stage makes it; the NaN rows give NaN slots), with M candidates and with the first one alone; every third image's count
        // is 0 (an invalid crop).  The same bits at 1 and 4 threads, with and without a report, into exactly sized buffers; mode 0
        // is esahrnet_pnp_batch_cand, mode 1 esahrnet_pnp_batch_cand_w on the rows, bit for bit, and a count-0 image the NaN row
        for (int mode = 0; mode < 2; ++mode)
            for (int Mr : {M, 1}) {
                std::vector<double> cpts, cw;
                std::vector<float> cpeak;
                std::vector<int32_t> count, order;
                make_record(cand, hess, m, k, M, Mr, boxes, rates, sel[0], (int)sel[1], mode, cpts, cw, cpeak, count, order);
                std::vector<double> qr0, tr0, repr0;
                std::vector<int32_t> usedr0;
                for (int threads : {1, 4})
                    for (int with_report = 0; with_report < 2; ++with_report) {
                        std::vector<double> q((size_t)m * 4), t((size_t)m * 3), rep(with_report ? m * R : 0);
                        std::vector<int32_t> used((size_t)m * k);
                        if (esahrnet_pnp_batch_cand_pts(cpts.data(), cw.data(), cpeak.data(), count.data(), order.data(), m, k, Mr,
                                                        kp3d.data(), K9.data(), sel[2], threads, q.data(), t.data(),
                                                        with_report ? rep.data() : nullptr, used.data())) {
                            std::fprintf(stderr, "candidate record %d: %s\n", nrec, esa::g_err);
                            return 1;
                        }
                        if (qr0.empty()) { qr0 = q; tr0 = t; usedr0 = used; }
                        if (with_report && repr0.empty()) repr0 = rep;
                        if (!same(q, qr0) || !same(t, tr0) || used != usedr0 || (with_report && !same(rep, repr0))) {
                            std::fprintf(stderr, "candidate record %d: record results differ (mode %d, M %d, threads %d, report %d)\n", nrec,
                                         mode, Mr, threads, with_report);
                            return 1;
                        }
                    }
                // the rows' own solve: the first Mr candidates of every keypoint, their Hessians in mode 1
                std::vector<float> rows((size_t)m * k * Mr * 3);
                std::vector<double> hrows((size_t)m * k * Mr * 3), qa((size_t)m * 4), ta((size_t)m * 3), ra(m * R);
                std::vector<int32_t> ua((size_t)m * k);
                for (size_t i = 0; i < (size_t)m * k; ++i) {
                    std::memcpy(&rows[i * Mr * 3], &cand[i * M * 3], (size_t)Mr * 3 * sizeof(float));
                    std::memcpy(&hrows[i * Mr * 3], &hess[i * M * 3], (size_t)Mr * 3 * sizeof(double));
                }
                if (esahrnet_pnp_batch_cand_w(rows.data(), mode ? hrows.data() : nullptr, m, k, Mr, kp3d.data(), K9.data(), boxes.data(),
                                              rates.data(), sel[0], (int)sel[1], sel[2], 1, qa.data(), ta.data(), ra.data(), ua.data())) {
                    std::fprintf(stderr, "candidate record %d: %s\n", nrec, esa::g_err);
                    return 1;
                }
                for (int i = 0; i < m; ++i) {
                    bool ok;
                    if (count[i] == 0) {
                        ok = std::isnan(qr0[i * 4]) && std::isnan(tr0[i * 3]) && repr0[i * R + ESAHRNET_REPORT_STATUS] == 1.0 &&
                             repr0[i * R + ESAHRNET_REPORT_N] == 0.0;
                        for (int j = 0; j < k; ++j) ok = ok && usedr0[(size_t)i * k + j] == -1;
                    } else {
                        ok = !std::memcmp(&qr0[i * 4], &qa[i * 4], 4 * sizeof(double)) && !std::memcmp(&tr0[i * 3], &ta[i * 3], 3 * sizeof(double)) &&
                             !std::memcmp(&repr0[i * R], &ra[i * R], R * sizeof(double)) &&
                             !std::memcmp(&usedr0[(size_t)i * k], &ua[(size_t)i * k], k * sizeof(int32_t));
                    }
                    if (!ok) {
                        std::fprintf(stderr, "candidate record %d image %d: the solve on the record is not the solve on the rows (mode %d, M %d)\n",
                                     nrec, i, mode, Mr);
                        return 1;
                    }
                }
            }
        int rescued = 0, swaps = 0, solved = 0;
        for (int i = 0; i < m; ++i) {
            int s = 0;
            for (int j = 0; j < k; ++j) s += used0[(size_t)i * k + j] > 0;
            rescued += s > 0;
            swaps += s;
            solved += rep0[i * R + ESAHRNET_REPORT_STATUS] == 0;
        }
        std::printf("candidate record %d: %d images of %d keypoints x %d candidates, %d solved, %d rescued with %d swaps\n", nrec, m, k,
                    M, solved, rescued, swaps);
        ++nrec;
    }
    std::fclose(f);
    double q[4], t[3];
    int used[11];
    float c[11 * 3] = {0};
    double z[33] = {0};
    int b[2] = {0, 0};
    if (esahrnet_pnp_batch_cand(c, 1, 11, 5, z, z, b, z, 0.5, 0, 0.3, 1, q, t, nullptr, used) != 1 || !std::strstr(esa::g_err, "candidates") ||
        esahrnet_pnp_batch_cand(c, 1, 11, 1, z, z, b, z, 0.5, 0, -1.0, 1, q, t, nullptr, used) != 1 || !std::strstr(esa::g_err, "min_ratio") ||
        esahrnet_pnp_batch_cand(c, 1, 11, 1, z, z, b, z, 0.5, 0, 0.3, 1, q, t, nullptr, nullptr) != 1 || !std::strstr(esa::g_err, "null")) {
        std::fprintf(stderr, "a bad argument of esahrnet_pnp_batch_cand was not refused\n");
        return 1;
    }
    if (esahrnet_pnp_batch_cand_w(c, z, 1, 11, 5, z, z, b, z, 0.5, 0, 0.3, 1, q, t, nullptr, used) != 1 || !std::strstr(esa::g_err, "pnp_batch_cand_w") ||
        esahrnet_pnp_batch_cand_w(c, z, 1, 11, 1, z, z, b, z, 0.5, 0, -1.0, 1, q, t, nullptr, used) != 1 || !std::strstr(esa::g_err, "min_ratio") ||
        esahrnet_pnp_batch_cand_w(nullptr, z, 1, 11, 1, z, z, b, z, 0.5, 0, 0.3, 1, q, t, nullptr, used) != 1 || !std::strstr(esa::g_err, "null")) {
        std::fprintf(stderr, "a bad argument of esahrnet_pnp_batch_cand_w was not refused\n");
        return 1;
    }
    // esahrnet_pnp_batch_cand_pts: each refused argument, in the order of its checks (the next check would fire too)
    {
        double p[11 * 2] = {0}, w3[11 * 3] = {0};
        float pk[11] = {0};
        int cnt[1] = {4}, ord[11] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, over[1] = {12}, under[1] = {-1}, bad[11] = {0, 1, 2, 11};
        const auto refused = [&](int rc, const char* text) {
            return rc == 1 && std::strstr(esa::g_err, "pnp_batch_cand_pts") && std::strstr(esa::g_err, text);
        };
        if (!refused(esahrnet_pnp_batch_cand_pts(nullptr, w3, pk, cnt, ord, -1, 11, 1, z, z, 0.3, 1, q, t, nullptr, used), "null") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, nullptr, cnt, ord, -1, 11, 1, z, z, 0.3, 1, q, t, nullptr, used), "null") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, cnt, ord, 1, 11, 1, z, z, 0.3, 1, q, t, nullptr, nullptr), "null") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, cnt, ord, -1, 0, 1, z, z, 0.3, 1, q, t, nullptr, used), "negative image count") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, cnt, ord, 1, 65, 5, z, z, 0.3, 1, q, t, nullptr, used), "keypoints per image") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, cnt, ord, 1, 11, 5, z, z, -1.0, 1, q, t, nullptr, used), "candidates per keypoint") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, cnt, ord, 1, 11, 0, z, z, -1.0, 1, q, t, nullptr, used), "candidates per keypoint") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, over, ord, 1, 11, 1, z, z, NAN, 1, q, t, nullptr, used), "min_ratio") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, over, bad, 1, 11, 1, z, z, 0.3, 1, q, t, nullptr, used), "count[0] = 12") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, under, bad, 1, 11, 1, z, z, 0.3, 1, q, t, nullptr, used), "count[0] = -1") ||
            !refused(esahrnet_pnp_batch_cand_pts(p, w3, pk, cnt, bad, 1, 11, 1, z, z, 0.3, 1, q, t, nullptr, used), "order[0][3] = 11")) {
            std::fprintf(stderr, "a bad argument of esahrnet_pnp_batch_cand_pts was not refused: %s\n", esa::g_err);
            return 1;
        }
        // zero images: nothing is read or written
        if (esahrnet_pnp_batch_cand_pts(p, w3, pk, cnt, ord, 0, 11, 1, z, z, 0.3, 1, q, t, nullptr, used) != 0) {
            std::fprintf(stderr, "an empty batch was refused: %s\n", esa::g_err);
            return 1;
        }
    }
    std::printf("ok: %d candidate records\n", nrec);
    return nrec ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) { std::fprintf(stderr, "usage: %s records.bin [candidates.bin]\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t head[3];
    int nrec = 0;
    while (std::fread(head, sizeof(int32_t), 3, f) == 3) {
        const int m = head[0], k = head[1], has_kp = head[2];
        std::vector<double> pts, w, kp3d, K9, rates, sel;
        std::vector<int32_t> count, order, boxes;
        std::vector<float> kp;
        bool ok = read_vec(f, pts, (size_t)m * k * 2) && read_vec(f, w, (size_t)m * k * 3) && read_vec(f, count, m) &&
                  read_vec(f, order, (size_t)m * k) && read_vec(f, kp3d, (size_t)k * 3) && read_vec(f, K9, 9);
        if (ok && has_kp)
            ok = read_vec(f, kp, (size_t)m * k * 3) && read_vec(f, boxes, (size_t)m * 2) && read_vec(f, rates, m) && read_vec(f, sel, 2);
        if (!ok) { std::fprintf(stderr, "record %d is cut short\n", nrec); return 2; }
        const size_t R = ESAHRNET_POSE_REPORT_DOUBLES;
        for (int entry = 0; entry <= has_kp; ++entry) {
            std::vector<double> q0, t0, rep0;
            for (int threads : {1, 4})
                for (int form = 0; form < 3; ++form) {          // 0: the old entry, 1: _ex with a null report, 2: _ex with a report
                    // exact sizes, so that a write past a row's end is a heap overflow the sanitizer sees
                    std::vector<double> q((size_t)m * 4), t((size_t)m * 3), rep(form == 2 ? m * R : 0);
                    double* rp = form == 2 ? rep.data() : nullptr;
                    int rc;
                    if (entry == 0)
                        rc = form == 0 ? esahrnet_pnp_batch_w(pts.data(), w.data(), count.data(), m, k, kp3d.data(), order.data(),
                                                              K9.data(), threads, q.data(), t.data())
                                       : esahrnet_pnp_batch_w_ex(pts.data(), w.data(), count.data(), m, k, kp3d.data(), order.data(),
                                                                 K9.data(), threads, q.data(), t.data(), rp);
                    else
                        rc = form == 0 ? esahrnet_pnp_batch(kp.data(), m, k, kp3d.data(), K9.data(), boxes.data(), rates.data(),
                                                            sel[0], (int)sel[1], threads, q.data(), t.data())
                                       : esahrnet_pnp_batch_ex(kp.data(), m, k, kp3d.data(), K9.data(), boxes.data(), rates.data(),
                                                               sel[0], (int)sel[1], threads, q.data(), t.data(), rp);
                    if (rc) { std::fprintf(stderr, "record %d: %s\n", nrec, esa::g_err); return 1; }
                    if (q0.empty()) { q0 = q; t0 = t; }
                    if (!same(q, q0) || !same(t, t0)) {
                        std::fprintf(stderr, "record %d entry %d: poses differ (threads %d, form %d)\n", nrec, entry, threads, form);
                        return 1;
                    }
                    if (form == 2) {
                        if (rep0.empty()) rep0 = rep;
                        if (!same(rep, rep0)) {
                            std::fprintf(stderr, "record %d entry %d: report differs at %d threads\n", nrec, entry, threads);
                            return 1;
                        }
                    }
                }
            int solved = 0, nocov = 0, fallback = 0;
            for (int i = 0; i < m; ++i) {
                solved += rep0[i * R + ESAHRNET_REPORT_STATUS] == 0;
                nocov += rep0[i * R + ESAHRNET_REPORT_STATUS] == 0 && ((int)rep0[i * R + ESAHRNET_REPORT_FLAGS] & 2);
                fallback += rep0[i * R + ESAHRNET_REPORT_STATUS] == 0 && ((int)rep0[i * R + ESAHRNET_REPORT_FLAGS] & 1);
            }
            std::printf("record %d (%s): %d images, %d solved, %d without a covariance, %d on the no-consensus fallback\n", nrec,
                        entry ? "pnp_batch_ex" : "pnp_batch_w_ex", m, solved, nocov, fallback);
        }
        ++nrec;
    }
    std::fclose(f);
    // the argument checks, which answer through set_error
    double q[4], t[3];
    if (esahrnet_pnp_batch_w_ex(nullptr, nullptr, nullptr, 1, 11, nullptr, nullptr, nullptr, 1, q, t, nullptr) != 1 ||
        !std::strstr(esa::g_err, "null argument")) {
        std::fprintf(stderr, "a null argument was not refused\n");
        return 1;
    }
    std::printf("ok: %d records\n", nrec);
    if (!nrec) return 2;
    return argc == 3 ? check_candidates(argv[2]) : 0;
}
