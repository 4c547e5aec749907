// d2d_selftest.cpp -- csrc/gsr_d2d.h (the pair and row math of mixture-to-mixture registration) as a stand-alone
// program: six pairs of two source rows and three target rows against the numbers tests/d2d_model.py gives for them (per pair exactly,
// the 32 sums to rounding), a singular pair with and without the floor, and the refusals of the scalar arguments.  Built with
// -fsanitize=address,undefined by tests/test_d2d_cpu.py; nothing of the library is linked.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/d2d_selftest.cpp -o d2d_selftest && ./d2d_selftest
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../gaussiansplattingregistration_amd/csrc/gsr_d2d.h"

using namespace gsr::d2d;

static int failures = 0;
#define EXPECT(cond, what)                                                   \
    do {                                                                     \
        if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); ++failures; } \
    } while (0)

// ---- inputs and the model's numbers (tests/d2d_model.py: pair_terms and accumulate, max_corr = 10: every pair counts)
static const float SX[6] = {0x1.00320ep-2f, 0x1.96bf36p-1f, 0x1.1a4d5ap-1f, -0x1.19634ap-1f, -0x1.99426cp-2f, 0x1.7e84ccp-1f};
static const float SA[12] = {0x1.a9f252p-6f, 0x1.9b01fcp-7f, 0x1.d00938p-7f, 0x1.673354p-4f, 0x1.0328dp-6f, 0x1.2cb0ecp-6f,
                             0x1.09fa44p-4f, -0x1.d8931ep-9f, 0x1.7ad2c2p-6f, 0x1.09abb2p-8f, 0x1.e2b7e6p-8f, 0x1.292108p-5f};
static const float SW[2] = {0x1.8p-1f, 0x1.8p+0f};
static const float TX[9] = {0x1.03465ep-2f, 0x1.b90e72p-1f, 0x1.0db3ap-1f, -0x1.2945a2p-1f, -0x1.802df6p-2f, 0x1.87a7b2p-1f, 0x1.0597bep-2f, 0x1.7eed4cp-1f, 0x1.198da6p-1f};
static const float TB[18] = {0x1.9ed0e4p-6f, 0x1.d67e2ep-7f, 0x1.99089ep-10f, 0x1.91032ap-7f, 0x1.5015a4p-11f, 0x1.51812ap-10f,
                             0x1.1addd2p-5f, 0x1.5bd31cp-6f, 0x1.43687p-6f, 0x1.09f2ccp-5f, 0x1.cb2b74p-6f, 0x1.a150eap-5f,
                             0x1.336ea6p-6f, 0x1.392c66p-9f, -0x1.62c582p-7f, 0x1.8d6e04p-8f, 0x1.275b9ep-7f, 0x1.f72abp-6f};
static const float TV[3] = {0x1.0p+0f, 0x1.0p-1f, 0x1.0p+1f};
static const double TM[16] = {0x1.fc4f935722b64p-1, 0x1.76b965428deedp-5, 0x1.c5a60befbc438p-4, 0x1.eb851eb851eb8p-6,
                              -0x1.625ec7234d727p-5, 0x1.ff5d2b0f05fc2p-1, -0x1.954152716ea95p-6, -0x1.47ae147ae147bp-6,
                              -0x1.c9b82b8f95f60p-4, 0x1.43d6d9f46cb7fp-6, 0x1.fcb1464e1f1f0p-1, 0x1.999999999999ap-5,
                              0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p+0};
static const double COV_SCALE = 0x1.8000000000000p+0, COV_FLOOR = 0x1.a36e2eb1c432dp-14;
// per pair, in the order (0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)
static const double WANT_M[36] = {0x1.7163ef5dba595p+3, -0x1.281a31582a4fdp+1, -0x1.08b5ddbb87cfcp+3, 0x1.7201d5c86bee8p+2, -0x1.9a4616e4361fap+1, 0x1.216080231400dp+5,
                                  0x1.3aa638e36ea0bp+3, -0x1.bf9b6b9a94890p+0, -0x1.e97abd8d8d055p+1, 0x1.4e98e451791a6p+2, -0x1.3eec6ce688834p+1, 0x1.45b2232dd95b6p+3,
                                  0x1.3a4560c66ed7ep+3, -0x1.12db00aef0bf8p+1, 0x1.d1692256bb6bcp-2, 0x1.849819366d9cep+2, -0x1.7f97282e42309p+1, 0x1.617bd47b373f4p+3,
                                  0x1.62d48224a3fa0p+2, -0x1.6610d90e83922p+0, -0x1.a030b306f5671p+1, 0x1.df1e3946acaffp+4, -0x1.577c79c0232c0p+2, 0x1.09ec41727be3dp+4,
                                  0x1.4e48e59b2fbf7p+2, 0x1.232af0b118215p-2, -0x1.4ce963f99e9d4p+1, 0x1.3caf534cacca6p+4, -0x1.0adaa4b199b70p+3, 0x1.41fef30d0e8c7p+3,
                                  0x1.5cceda37c7813p+2, 0x1.3a35a25efd72cp+2, -0x1.f7587dff02439p+0, 0x1.21090c005f85cp+6, -0x1.25cfff2116597p+4, 0x1.7bf6f63f9c1b8p+3};
static const double WANT_MR[18] = {0x1.30617c6ff3dedp+0, -0x1.1f492a088ae91p+0, 0x1.791489a896b7ep+0, 0x1.03fcb1ffc82eap+3, 0x1.29b9185c24255p+2, -0x1.09180ced41042p+3,
                                   0x1.321790fdad494p+0, -0x1.6f49d3cb5ce11p-2, 0x1.c7e5d5bfb1197p-2, -0x1.9450039025046p+1, -0x1.375467aaf4c15p+5, 0x1.cdfdab8d56954p+3,
                                   0x1.d1c5d0ed69d02p-2, -0x1.6743a25951857p+0, 0x1.995eaac82052ap-1, -0x1.4460431565f08p+3, -0x1.7367ffdbcd9f9p+6, 0x1.a3c9ec08a6b4cp+4};
static const double WANT_m[6] = {0x1.6f2c1f8647d34p-2, 0x1.cf8da1d088287p+3, 0x1.465f7d9cdd5bcp-3, 0x1.c3b0a73856c33p+5, 0x1.6c32dd18bd800p-3, 0x1.eb32549770bf8p+6};
static const double WANT_OMEGA[6] = {0x1.40f94422e587cp-1, 0x1.19354367932e0p-12, 0x1.6296fd71ca1b4p+0, 0x1.cf9cc2691b33ap-41, 0x1.5f548fb7a9b28p-1, 0x1.00ba7dc19802cp-87};
static const double WANT_SUMS[32] = {0x1.2dd44a820079cp+5, -0x1.64b901eb59e98p+3, 0x1.2b78afd63b66cp-1, -0x1.fd533e67c1ad0p-3, -0x1.4c7f584debdb5p+4, 0x1.1049251b143c8p+5,
                                     0x1.11f7381f1e0c3p+4, -0x1.107edbceea26ep+3, 0x1.024aa7157fe04p+4, -0x1.58a1faf88b1fdp+1, -0x1.eabbbe64c1b1ap+3, 0x1.3302ec61190ecp+4,
                                     -0x1.fc193507d54b2p+3, 0x1.ca5976cde6128p+0, 0x1.78772edf073aap+1, 0x1.86d3249838dcap+4, -0x1.0eb5ab7cc2571p+2, -0x1.95e401b5b9155p+2,
                                     0x1.99e170cda11fcp+4, -0x1.7c43a3f6a6decp+3, 0x1.671314a2b439dp+5, 0x1.387ebfc3b5f10p+1, 0x1.575209fb1d2d8p+0, -0x1.aff24c3b3b4c8p+0,
                                     0x1.5ba0055f46721p+1, -0x1.14be9b5dcf15dp+1, 0x1.0b12800b0b388p+1, 0x1.5967bd59a48cap+1, 0x1.2492c1a6d91dcp-1, 0x1.8000000000000p+2,
                                     0x1.0000000000000p+1, 0x0.0p+0};

int main() {
    const int NS = 2, NT = 3;
    const double s2 = COV_SCALE * COV_SCALE;
    double sums[SUMS_LEN];
    for (int k = 0; k < SUMS_LEN; ++k) sums[k] = 0.0;
    int pair = 0;
    for (int i = 0; i < NS; ++i) {
        double p[3], A[6], S[6];
        move_point(TM, (double)SX[3 * i], (double)SX[3 * i + 1], (double)SX[3 * i + 2], p);
        for (int k = 0; k < 6; ++k) A[k] = (double)SA[6 * i + k];
        rotate_cov(TM, A, S);
        RowAcc acc;
        for (int j = 0; j < NT; ++j, ++pair) {
            const double r[3] = {p[0] - (double)TX[3 * j], p[1] - (double)TX[3 * j + 1], p[2] - (double)TX[3 * j + 2]};
            double B[6], M[6], Mr[3], m = 0.0;
            for (int k = 0; k < 6; ++k) B[k] = (double)TB[6 * j + k];
            EXPECT(pair_metric(S, B, s2, COV_FLOOR, r, M, Mr, &m), "a regular pair");
            for (int k = 0; k < 6; ++k) EXPECT(M[k] == WANT_M[6 * pair + k], "M");
            for (int k = 0; k < 3; ++k) EXPECT(Mr[k] == WANT_MR[3 * pair + k], "M r");
            EXPECT(m == WANT_m[pair], "m");
            const double wv = (double)SW[i] * (double)TV[j], e = exp(-0.5 * m);
            EXPECT(fabs(wv * e - WANT_OMEGA[pair]) <= 4.0 * 2.220446049250313e-16 * WANT_OMEGA[pair], "omega");
            row_add(acc, wv, e, M, Mr, m);
        }
        double row[SUMS_LEN];
        row_expand(p, acc, row);
        for (int k = 0; k < SUMS_LEN; ++k) sums[k] += row[k];
    }
    double scale = 0.0;
    for (int k = 0; k < 27; ++k) scale = fmax(scale, fabs(WANT_SUMS[k]));
    for (int k = 0; k < 29; ++k) EXPECT(fabs(sums[k] - WANT_SUMS[k]) <= 1e-13 * scale, "a sum");
    for (int k = 29; k < 32; ++k) EXPECT(sums[k] == WANT_SUMS[k], "a count");

    // zero covariances: singular without the floor, regular with it (M = I / phi)
    {
        const double Z[6] = {0, 0, 0, 0, 0, 0}, r[3] = {0.5, -0.25, 0.125};
        double M[6] = {-1, -1, -1, -1, -1, -1}, Mr[3], m = -1.0;
        EXPECT(!pair_metric(Z, Z, 1.0, 0.0, r, M, Mr, &m), "zero covariances, no floor");
        EXPECT(M[0] == -1.0 && m == -1.0, "a singular pair writes nothing");
        EXPECT(pair_metric(Z, Z, 1.0, 0.25, r, M, Mr, &m), "zero covariances, floor");
        EXPECT(M[0] == 4.0 && M[3] == 4.0 && M[5] == 4.0 && M[1] == 0.0 && M[2] == 0.0 && M[4] == 0.0, "M = I / phi");
        EXPECT(m == 4.0 * (0.25 + 0.0625 + 0.015625), "m = |r|^2 / phi");
        const double N[6] = {-1.0, 0, 0, 1.0, 0, 1.0};                     // an indefinite matrix: det < 0
        EXPECT(!pair_metric(N, Z, 1.0, 0.0, r, M, Mr, &m), "negative determinant");
        const double big[6] = {1e200, 0, 0, 1e200, 0, 1e200};               // det overflows
        EXPECT(!pair_metric(big, Z, 1.0, 0.0, r, M, Mr, &m), "infinite determinant");
    }
    // a row without pairs: thirty-two zeros
    {
        const double p[3] = {1.0, 2.0, 3.0};
        RowAcc acc;
        double row[SUMS_LEN];
        row_expand(p, acc, row);
        for (int k = 0; k < SUMS_LEN; ++k) EXPECT(row[k] == 0.0, "an empty row");
    }
    // the scalar arguments
    {
        double T[16];
        memcpy(T, TM, sizeof T);
        EXPECT(check_scalars(T, 1.0, 0.0)[0] == 0, "valid arguments");
        EXPECT(check_scalars(nullptr, 1.0, 0.0)[0] != 0, "NULL T");
        EXPECT(check_scalars(T, 0.0, 0.0)[0] != 0, "cov_scale 0");
        EXPECT(check_scalars(T, -1.0, 0.0)[0] != 0, "cov_scale < 0");
        EXPECT(check_scalars(T, NAN, 0.0)[0] != 0, "cov_scale NaN");
        EXPECT(check_scalars(T, INFINITY, 0.0)[0] != 0, "cov_scale inf");
        EXPECT(check_scalars(T, 1.0, -1e-9)[0] != 0, "cov_floor < 0");
        EXPECT(check_scalars(T, 1.0, NAN)[0] != 0, "cov_floor NaN");
        EXPECT(check_scalars(T, 1.0, INFINITY)[0] != 0, "cov_floor inf");
        T[7] = NAN;
        EXPECT(check_scalars(T, 1.0, 0.0)[0] != 0, "T NaN");
        T[7] = INFINITY;
        EXPECT(check_scalars(T, 1.0, 0.0)[0] != 0, "T inf");
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
