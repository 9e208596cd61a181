// consensus_math_main.cpp -- a stand-alone program over sr_livo_amd/csrc/srl_consensus_math.h compiled as plain C++ (the header says it
// does): tests/test_consensus_math.py builds it with the host compiler, once plain and once with -fsanitize=address,undefined, feeds it
// cases and compares what it prints with the checker, np.roots and known poses.  One case per input line (stdin, or the file named as
// the only argument), one answer line per case, every number as %.17g:
//   sample S seed h m              ->  1|0 then the S positions (-1 where none)
//   cubic c0 c1 c2 c3              ->  the count then the three slots (nan: no root)
//   quartic c0 ... c4              ->  the count then the four slots
//   seven N[6] then 7 x (x1 y1 x2 y2)  ->  -1 (no null space: rank below 7) or the number of models, then 9 numbers per model
//                                      (the kernel's sequence: normalise, 7 x 9 rows, null space, det cubic, roots, de-normalise)
//   p3p P[9] J[9]                  ->  the number of poses, then 12 numbers per pose
// No device call and nothing of Python in the process.
#include "../sr_livo_amd/csrc/srl_consensus_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static bool numbers(char *p, std::vector<double> &v) {
    v.clear();
    for (;;) {
        char *end = nullptr;
        const double x = std::strtod(p, &end);
        if (end == p) break;
        v.push_back(x);
        p = end;
    }
    while (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t') p++;
    return *p == 0;
}

static void put(double x) {
    if (std::isnan(x)) std::printf(" nan");
    else std::printf(" %.17g", x);
}

template <int S>
static void do_sample(const std::vector<double> &v) {
    int pos[S];
    const bool ok = cons_sample<S>((uint32_t)v[1], (uint32_t)v[2], (int)v[3], pos);
    std::printf("%d", ok ? 1 : 0);
    for (int k = 0; k < S; k++) std::printf(" %d", pos[k]);
    std::printf("\n");
}

static int do_seven(const std::vector<double> &v) {
    const double *N = v.data(), *p = v.data() + 6;
    double W[81];
    for (int r = 0; r < 7; r++) {
        const double x1 = N[2] * (p[4 * r] - N[0]), y1 = N[2] * (p[4 * r + 1] - N[1]);
        const double x2 = N[5] * (p[4 * r + 2] - N[3]), y2 = N[5] * (p[4 * r + 3] - N[4]);
        double *row = W + 9 * r;
        row[0] = x2 * x1; row[1] = x2 * y1; row[2] = x2; row[3] = y2 * x1; row[4] = y2 * y1; row[5] = y2; row[6] = x1; row[7] = y1; row[8] = 1.0;
    }
    if (!cons_nullspace_7x9(W, 1)) { std::printf("-1\n"); return 0; }
    double c[4], root[3], F[3][9];
    cons_det_cubic(W + 63, W + 72, c);
    cons_cubic(c, root);
    int nm = 0;
    for (int m = 0; m < 3; m++) {
        if (!std::isfinite(root[m])) continue;
        double Fn[9];
        for (int k = 0; k < 9; k++) Fn[k] = root[m] * W[63 + k] + (1.0 - root[m]) * W[72 + k];
        if (cons_denormalise(Fn, N, F[nm])) nm++;
    }
    std::printf("%d", nm);
    for (int m = 0; m < nm; m++) for (int k = 0; k < 9; k++) put(F[m][k]);
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    FILE *in = stdin;
    if (argc > 1) {
        in = std::fopen(argv[1], "r");
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    }
    std::vector<char> line(1 << 16);
    std::vector<double> v;
    int cases = 0;
    while (std::fgets(line.data(), (int)line.size(), in)) {
        char *p = line.data();
        while (*p == ' ') p++;
        if (*p == 0 || *p == '\n' || *p == '#') continue;
        char *sp = std::strchr(p, ' ');
        const std::string cmd(p, sp ? (size_t)(sp - p) : std::strcspn(p, "\r\n"));
        if (!numbers(sp ? sp : p + cmd.size(), v)) { std::fprintf(stderr, "malformed case: %s", line.data()); return 2; }
        const size_t n = v.size();
        if (cmd == "sample" && n == 4 && (v[0] == 7.0 || v[0] == 3.0)) {
            if (v[0] == 7.0) do_sample<7>(v); else do_sample<3>(v);
        } else if (cmd == "cubic" && n == 4) {
            double r[3];
            std::printf("%d", cons_cubic(v.data(), r));
            for (int k = 0; k < 3; k++) put(r[k]);
            std::printf("\n");
        } else if (cmd == "quartic" && n == 5) {
            double r[4];
            std::printf("%d", cons_quartic(v.data(), r));
            for (int k = 0; k < 4; k++) put(r[k]);
            std::printf("\n");
        } else if (cmd == "seven" && n == 6 + 28) {
            do_seven(v);
        } else if (cmd == "p3p" && n == 18) {
            double out[48];
            const int np = cons_p3p(v.data(), v.data() + 9, out);
            std::printf("%d", np);
            for (int k = 0; k < 12 * np; k++) put(out[k]);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown case: %s", line.data());
            return 2;
        }
        cases++;
    }
    if (in != stdin) std::fclose(in);
    std::printf("consensus math: %d cases\n", cases);
    return 0;
}
