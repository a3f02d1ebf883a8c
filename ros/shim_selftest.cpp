// Compiles the MatchGPULib shim without OpenCV/ROS (a struct with the same field names stands in
// for cv_bridge::CvImagePtr) and runs one small full-mode and one foveated match through it.
//   g++ -std=c++17 -Iinclude ros/shim_selftest.cpp -Lug_stereomatcher_amd -lugsm -Wl,-rpath,$PWD/ug_stereomatcher_amd
#include <cstdint>
#include <memory>
#include <vector>

#include "MatchGPULib_ugsm.hpp"

struct Mat { int rows, cols; size_t step; unsigned char *data; };
struct CvImage { Mat image; };
typedef std::shared_ptr<CvImage> CvImagePtr;

int main(int argc, char **argv)
{
    const int W = 320, H = 240;
    std::vector<uint8_t> l(3 * W * H), r(3 * W * H);
    unsigned s = 1;
    for (size_t i = 0; i < l.size(); i++) { s = s * 1664525u + 1013904223u; l[i] = 1 + (s >> 24) % 255; }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            for (int c = 0; c < 3; c++) r[(y * W + x) * 3 + c] = l[(y * W + (x >= 2 ? x - 2 : 0)) * 3 + c];
    CvImagePtr L(new CvImage{{H, W, (size_t)3 * W, l.data()}}), R(new CvImage{{H, W, (size_t)3 * W, r.data()}});
    char *av[] = {(char *)"node", (char *)"x", (char *)"3"};
    try {
        MatchGPULib m(3, av);
        m.initStack(L, R);
        std::printf("fovea %dx%d levels %d\n", m.getFoveaWidth(), m.getFoveaHeight(), m.getFoveateLevel());
        float ***st = m.matchStack(L, R);
        if (!st) return 2;
        std::printf("stack[0][0][centre] = %f\n", st[0][0][(m.getFoveaHeight() / 2) * m.getFoveaWidth() + m.getFoveaWidth() / 2]);
        // match(L, R, 1) == matchStack + hierarchicalDisparity (MatchGPULib.cpp:354-360)
        float **full = m.hierarchicalDisparity(nullptr, st, 3, W, H);
        float **one = m.match(L, R, 1);
        if (!full || !one) return 3;
        size_t diff = 0;
        for (int c = 0; c < 3; c++) diff += std::memcmp(full[c], one[c], sizeof(float) * W * H) != 0;
        std::printf("hierarchicalDisparity vs match(fov=1): %s, dx[centre] = %f, dx[corner] = %f\n", diff ? "DIFFER" : "identical",
                    full[0][(H / 2) * W + W / 2], full[0][0]);
        for (int c = 0; c < 3; c++) { free(full[c]); free(one[c]); }
        free(full);
        free(one);
        // the pipelined calls ("-inflight=3"): five frames enqueued, results in arrival order, equal to the blocking calls
        {
            char *av2[] = {(char *)"node", (char *)"x", (char *)"3", (char *)"-inflight=3"};
            MatchGPULib p(4, av2);
            float **blocking = p.match(L, R, 0);
            if (!blocking) return 4;
            size_t bad = 0, got = 0;
            uint64_t expect_tag = 0;
            MatchGPULib::Done d;
            auto check = [&](const MatchGPULib::Done &dn) {
                bad += dn.tag != expect_tag++;
                if (!dn.foveated) for (int c = 0; c < 3; c++) bad += std::memcmp(dn.planes[c], blocking[c], sizeof(float) * W * H) != 0;
                else for (int k = 0; k < p.getFoveateLevel(); k++)
                    for (int c = 0; c < 3; c++)
                        bad += std::memcmp(dn.planes[c] + (size_t)k * p.getFoveaWidth() * p.getFoveaHeight(), st[k][c], sizeof(float) * p.getFoveaWidth() * p.getFoveaHeight()) != 0;
                got++;
            };
            for (uint64_t t = 0; t < 5; t++) {
                if ((t & 1 ? p.enqueueStack(L, R, false, t) : p.enqueueMatch(L, R, t)) != UGSM_OK) return 5;
                while (p.outstanding() >= p.frames_in_flight) { if (!p.nextDone(true, &d)) return 6; check(d); }
            }
            while (p.outstanding() > 0) { if (!p.nextDone(true, &d)) return 7; check(d); }
            std::printf("pipelined (3 in flight) vs blocking: %zu frames, %s\n", got, bad ? "DIFFER" : "identical");
            for (int c = 0; c < 3; c++) free(blocking[c]);
            free(blocking);
            if (bad || got != 5) return 8;
        }
        // matchStackMulti: three windows of the pair in one call; the centred one is matchStack's, and level F-1 is the same in all
        {
            const int ox[3] = {40, 0, -5000}, oy[3] = {-25, 0, 5000};
            float ***multi[3];
            if (!m.matchStackMulti(L, R, 3, ox, oy, multi)) return 9;
            const int F = m.getFoveateLevel();
            const size_t fb = sizeof(float) * m.getFoveaWidth() * m.getFoveaHeight();
            size_t bad = 0;
            for (int k = 0; k < F; k++)
                for (int c = 0; c < 3; c++) bad += std::memcmp(multi[1][k][c], st[k][c], fb) != 0;
            for (int w = 0; w < 3; w++)
                for (int c = 0; c < 3; c++) bad += std::memcmp(multi[w][F - 1][c], st[F - 1][c], fb) != 0;
            std::printf("matchStackMulti (3 windows) vs matchStack: %s\n", bad ? "DIFFER" : "identical");
            for (int w = 0; w < 3; w++) {
                for (int k = 0; k < F; k++) { for (int i = 0; i < 3; i++) free(multi[w][k][i]); free(multi[w][k]); }
                free(multi[w]);
            }
            if (bad) return 10;
        }
        // matchStackMulti with a tau: the centred window is matchStack's under setLRCheck(tau, 2), and the context's setting stays off
        {
            const int ox[3] = {40, 0, -5000}, oy[3] = {-25, 0, 5000};
            float ***multi[3];
            if (!m.matchStackMulti(L, R, 3, ox, oy, multi, 1.0f)) return 11;
            if (m.setLRCheck(1.0f, 2) != UGSM_OK) return 12;
            float ***chk = m.matchStack(L, R);
            if (m.setLRCheck(0.0f, 0) != UGSM_OK || !chk) return 13;
            const int F = m.getFoveateLevel();
            const size_t fb = sizeof(float) * m.getFoveaWidth() * m.getFoveaHeight();
            size_t bad = 0, zeroed = 0;
            for (int k = 0; k < F; k++) {
                for (int c = 0; c < 3; c++) bad += std::memcmp(multi[1][k][c], chk[k][c], fb) != 0;
                zeroed += std::memcmp(chk[k][2], st[k][2], fb) != 0;
            }
            std::printf("matchStackMulti (3 windows, tau 1) vs checked matchStack: %s; levels the check changed: %zu\n", bad ? "DIFFER" : "identical", zeroed);
            for (int w = 0; w < 3; w++) {
                for (int k = 0; k < F; k++) { for (int i = 0; i < 3; i++) free(multi[w][k][i]); free(multi[w][k]); }
                free(multi[w]);
            }
            for (int k = 0; k < F; k++) { for (int i = 0; i < 3; i++) free(chk[k][i]); free(chk[k]); }
            free(chk);
            if (bad) return 14;
        }
        // warpRightImage (MatchGPULib.cpp:1445-1518): the right image is the left one moved by two pixels, so under dx = 2, dy = 0 it lands
        // on the left image wherever the fetch stays inside the frame (columns 0 .. W-3)
        {
            const size_t n = (size_t)W * H;
            std::vector<float> planes(3 * n), left(3 * n), field(2 * n, 0.0f);
            for (size_t i = 0; i < n; i++) {
                field[i] = 2.0f;
                for (int c = 0; c < 3; c++) { planes[c * n + i] = r[3 * i + c]; left[c * n + i] = l[3 * i + c]; }
            }
            float *right[3] = {planes.data(), planes.data() + n, planes.data() + 2 * n}, *disp[2] = {field.data(), field.data() + n};
            float **warped = m.warpRightImage(right, disp, 3, W, H);
            if (!warped) return 15;
            size_t bad = 0;
            for (int c = 0; c < 3; c++)
                for (int y = 0; y < H; y++) bad += std::memcmp(warped[c] + (size_t)y * W, left.data() + c * n + (size_t)y * W, sizeof(float) * (W - 2)) != 0;
            std::printf("warpRightImage by dx = 2 vs the left image: %s\n", bad ? "DIFFER" : "identical");
            for (int c = 0; c < 3; c++) free(warped[c]);
            free(warped);
            if (bad) return 16;
        }
        // match(L, R, 0, tau): the left camera's field is match(L, R, 0)'s under setLRCheck(tau, 1), the right camera's match(R, L, 0)'s
        {
            float **bk = nullptr;
            float **chk = m.match(L, R, 0, 1.0f, &bk);
            if (!chk || !bk) return 17;
            if (m.setLRCheck(1.0f, 1) != UGSM_OK) return 18;
            float **seq = m.match(L, R, 0), **seqb = m.match(R, L, 0);
            if (m.setLRCheck(0.0f, 0) != UGSM_OK || !seq || !seqb) return 19;
            size_t bad = 0;
            for (int c = 0; c < 3; c++) bad += std::memcmp(chk[c], seq[c], sizeof(float) * W * H) != 0 || std::memcmp(bk[c], seqb[c], sizeof(float) * W * H) != 0;
            std::printf("match (tau 1, both directions in one call) vs the two checked matches: %s\n", bad ? "DIFFER" : "identical");
            for (float **p : {chk, bk, seq, seqb}) { for (int c = 0; c < 3; c++) free(p[c]); free(p); }
            if (bad) return 20;
        }
        // matchSeeded(L, R, prior, 5): the match started at level 5 from the cold result -- the same field every time, and not the cold one
        {
            float **cold = m.match(L, R, 0);
            if (!cold) return 21;
            float **s1 = m.matchSeeded(L, R, cold, 5), **s2 = m.matchSeeded(L, R, cold, 5);
            if (!s1 || !s2 || m.matchSeeded(L, R, cold, 14)) return 22;  // (level 14 does not exist: refused)
            size_t differ = 0, moved = 0;
            for (int c = 0; c < 3; c++) {
                differ += std::memcmp(s1[c], s2[c], sizeof(float) * W * H) != 0;
                moved += std::memcmp(s1[c], cold[c], sizeof(float) * W * H) != 0;
            }
            std::printf("matchSeeded (level 5 from the cold result) twice: %s; planes that differ from the cold match: %zu\n", differ ? "DIFFER" : "identical", moved);
            for (float **p : {cold, s1, s2}) { for (int c = 0; c < 3; c++) free(p[c]); free(p); }
            if (differ) return 23;
        }
        // matchCoarse(L, R, 5) then matchFine from its state: the cold match bit for bit; the prolongation has the images' size
        {
            float **cold = m.match(L, R, 0), **full = nullptr;
            if (!cold) return 24;
            float **state = m.matchCoarse(L, R, 5, &full);
            if (!state || !full || m.matchCoarse(L, R, 14)) return 25;  // (level 14 does not exist: refused)
            float **fin = m.matchFine(L, R, state, 5);
            if (!fin || m.matchFine(L, R, state, 0)) return 26;         // (level 0 is no state: refused)
            size_t differ = 0;
            for (int c = 0; c < 3; c++) differ += std::memcmp(fin[c], cold[c], sizeof(float) * W * H) != 0;
            std::printf("matchCoarse (level 5) + matchFine against match: %s\n", differ ? "DIFFER" : "identical");
            for (float **p : {cold, full, state, fin}) { for (int c = 0; c < 3; c++) free(p[c]); free(p); }
            if (differ) return 27;
        }
        // matchStackSeeded(L, R, st, {0, 0}, {12, -8}, F - 1): the window moved by a few pixels, started at the top fovea level from the cold stack --
        // the same stack every time; a start level that does not exist is refused
        {
            const int at0[2] = {0, 0}, at1[2] = {12, -8}, sl = m.getFoveateLevel() - 1;
            float ***w1 = m.matchStackSeeded(L, R, st, at0, at1, sl), ***w2 = m.matchStackSeeded(L, R, st, at0, at1, sl);
            if (!w1 || !w2 || m.matchStackSeeded(L, R, st, at0, at1, m.getFoveateLevel())) return 24;
            const size_t fn = (size_t)m.getFoveaWidth() * m.getFoveaHeight();
            size_t differ = 0;
            for (int k = 0; k < m.getFoveateLevel(); k++)
                for (int c = 0; c < 3; c++) differ += std::memcmp(w1[k][c], w2[k][c], sizeof(float) * fn) != 0;
            std::printf("matchStackSeeded (fovea level %d from the cold stack, window moved) twice: %s\n", sl, differ ? "DIFFER" : "identical");
            for (float ***p : {w1, w2}) {
                for (int k = 0; k < m.getFoveateLevel(); k++) { for (int c = 0; c < 3; c++) free(p[k][c]); free(p[k]); }
                free(p);
            }
            if (differ) return 25;
        }
        for (int k = 0; k < m.getFoveateLevel(); k++) { for (int i = 0; i < 3; i++) free(st[k][i]); free(st[k]); }
        free(st);
    } catch (const std::exception &e) {
        std::printf("no device: %s\n", e.what());
        return 0;
    }
    return 0;
}
