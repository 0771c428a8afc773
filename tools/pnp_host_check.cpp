// pnp_host_check.cpp — the host pose solver (csrc/pnp_host.hip) as a stand-alone program, for runs under host sanitizers.
//
// Links pnp_host.hip alone (the error text of plan.hip is restated below) and runs every record of a file that
// tools/pnp_host_check.py wrote through esahrnet_pnp_batch_w_ex (and esahrnet_pnp_batch_ex where the record has keypoint
// rows), with 1 and 4 threads, with and without a report buffer.  It checks what tests/test_pose_report_host.py checks at the
// C level: the poses do not depend on the report or the thread count, nor do the report's bits, and the old entries are the
// new ones with a null report.  A second file holds candidate records for esahrnet_pnp_batch_cand: the same bits at 1 and 4
// threads, with and without a report, and with one candidate the bits of esahrnet_pnp_batch_ex.  Exit status 0 and "ok" when
// all of it holds.  Pure host code: no GPU is touched.
//
// Build and run (tools/pnp_host_check.py does both):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/pnp_host_check.cpp esa-pose-estimation_amd/csrc/pnp_host.hip -fsanitize=address,undefined -o pnp_host_check
//   ./pnp_host_check records.bin candidates.bin
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/esahrnet.h"

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
