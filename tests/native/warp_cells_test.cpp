// Host walk of the Warper's cell and tap arithmetic (simplenerf_amd/csrc/warp_cells.h on splat_cells.h), built by the CPU suite with
// AddressSanitizer + UBSan (tests/test_warp_host.py).
//     warp_cells_test <h> <w> <c> <in.f64> <out.f64>
// in:  doubles: planes X, Y, Z of the sources (3 h w) | their values (h w c) | padded positions X, Y of the backward warp (2 h w) |
//      frame2 (h w c) | mask2 as 0 / 1 (h w) -- any values, non-finite included
// out: doubles: the splat sum v weight / sum weight or 0 (h w c) | sum weight (h w) | the backward warp nr / dr or 0 (h w c) | dr (h w)
// The splat keys every source, builds the inverted index with a stable counting sort and gathers every pixel through lists_of /
// corner_weights exactly as the kernel does; it checks that corner_weights hands out add_source's weights bit for bit and that the
// sums agree with a brute-force scatter into the padded grid.  The backward warp reads its taps through taps_of / frame_index from
// the unpadded frame and checks each against a brute-force zero-padded copy.  No index leaves its buffer (the sanitizers).  to_image
// is checked on the rounding ties.  Prints "warp_cells_test: OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../simplenerf_amd/csrc/warp_cells.h"

using namespace snerf::splat;

static int fail(const char* what, long long a, long long b) {
    std::printf("warp_cells_test: FAILED: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

int main(int argc, char** argv) {
    if (argc != 6) return fail("usage: h w c in out", argc, 0);
    const int h = std::atoi(argv[1]), w = std::atoi(argv[2]), c = std::atoi(argv[3]);
    if (h < 1 || w < 1 || c < 1 || c > 4) return fail("empty frame or channels outside 1..4", h, c);
    const long long n = (long long)h * w, total_in = 3 * n + n * c + 2 * n + n * c + n, total_out = n * c + n + n * c + n;
    double* in = new double[total_in];
    std::FILE* f = std::fopen(argv[4], "rb");
    if (!f || std::fread(in, sizeof(double), total_in, f) != (size_t)total_in) return fail("cannot read the input", 0, 0);
    std::fclose(f);
    const double *X = in, *Y = in + n, *Z = in + 2 * n, *values = in + 3 * n;
    const double *BX = values + n * c, *BY = BX + n, *frame2 = BY + n, *mask2 = frame2 + n * c;
    double* out = new double[total_out];
    double *splat = out, *weight_sum = out + n * c, *back = weight_sum + n, *back_dr = back + n * c;

    // ---- splat: keys, stable counting sort, gather
    const int discard = cell_keys(h, w), per_view = keys_per_view(h, w);
    int* keys = new int[n];
    double max_l = 0.0;
    for (long long i = 0; i < n; ++i) {
        keys[i] = source_key(X[i], Y[i], Z[i], h, w);
        if (keys[i] < 0 || keys[i] > discard) return fail("key out of range", i, keys[i]);
        max_l = std::fmax(max_l, log_depth(Z[i]));
    }
    int* starts = new int[per_view + 1]();
    for (long long i = 0; i < n; ++i) starts[keys[i] + 1] += 1;
    for (int k = 0; k < per_view; ++k) starts[k + 1] += starts[k];
    long long* order = new long long[n];
    int* cursor = new int[per_view];
    for (int k = 0; k < per_view; ++k) cursor[k] = starts[k];
    for (long long i = 0; i < n; ++i) order[cursor[keys[i]]++] = i;

    const long long padded = (long long)(h + 2) * (w + 2);
    double* sum_all = new double[padded * c]();
    double* ws_all = new double[padded]();
    if (max_l > 0.0) {
        for (long long i = 0; i < n; ++i) {
            if (keys[i] == discard && (!pinned(X[i]) || !pinned(Y[i]) || !is_finite(Z[i]))) continue;
            const Taps t = taps_of(X[i], Y[i], h, w);      // (the splat's corners are the backward warp's taps)
            const double d = depth_divisor(Z[i], max_l);
            for (int k = 0; k < 4; ++k) {
                if (t.row[k] < 0 || t.row[k] > h + 1 || t.col[k] < 0 || t.col[k] > w + 1) return fail("corner outside the padded grid", t.row[k], t.col[k]);
                const long long cell = (long long)t.row[k] * (w + 2) + t.col[k];
                for (int ch = 0; ch < c; ++ch) sum_all[cell * c + ch] += values[i * c + ch] * (t.prox[k] / d);
                ws_all[cell] += t.prox[k] / d;
            }
        }
    }
    for (int y = 0; y < h; ++y) {
        for (int x = 0; x < w; ++x) {
            double sum[4] = {0.0, 0.0, 0.0, 0.0}, ws = 0.0, zw_check = 0.0, ws_check = 0.0;
            if (max_l > 0.0) {
                int lists[4];
                const int num = lists_of(y + 1, x + 1, w, lists);
                for (int l = 0; l < num; ++l) {
                    if (lists[l] < 0 || lists[l] >= discard) return fail("a walked list is not a cell key", y, x);
                    for (int s = starts[lists[l]]; s < starts[lists[l] + 1]; ++s) {
                        const long long i = order[s];
                        double k[4];
                        const double d = depth_divisor(Z[i], max_l);
                        const int corners = corner_weights(X[i], Y[i], d, y + 1, x + 1, h, w, k);
                        if (corners < 0 || corners > 4) return fail("corner count", corners, i);
                        for (int j = 0; j < corners; ++j) {
                            for (int ch = 0; ch < c; ++ch) sum[ch] += values[i * c + ch] * k[j];
                            ws += k[j];
                        }
                        add_source(X[i], Y[i], values[i * c], d, y + 1, x + 1, h, w, zw_check, ws_check);
                    }
                }
            }
            // channel 0 through corner_weights is add_source's sum, bit for bit
            if (!same_bits(ws, ws_check) || !(same_bits(sum[0], zw_check) || (sum[0] != sum[0] && zw_check != zw_check)))
                return fail("corner_weights differs from add_source", y, x);
            const long long cell = (long long)(y + 1) * (w + 2) + (x + 1), pixel = (long long)y * w + x;
            if (std::fabs(ws - ws_all[cell]) > 1e-12 * std::fabs(ws_all[cell]) || (ws > 0.0) != (ws_all[cell] > 0.0))
                return fail("weight sum differs from the scatter", y, x);
            for (int ch = 0; ch < c; ++ch) {
                if (std::fabs(sum[ch] - sum_all[cell * c + ch]) > 1e-12 * std::fabs(ws_all[cell]) * 1000.0) return fail("value sum differs from the scatter", y, x);
                splat[pixel * c + ch] = ws > 0.0 ? sum[ch] / ws : 0.0;
            }
            weight_sum[pixel] = ws;
        }
    }

    // ---- backward warp: taps of the unpadded frame against a zero-padded copy
    double* frame_padded = new double[padded * c]();
    double* mask_padded = new double[padded]();
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const long long cell = (long long)(y + 1) * (w + 2) + (x + 1), pixel = (long long)y * w + x;
            for (int ch = 0; ch < c; ++ch) frame_padded[cell * c + ch] = frame2[pixel * c + ch];
            mask_padded[cell] = mask2[pixel] != 0.0 ? 1.0 : 0.0;
        }
    for (long long i = 0; i < n; ++i) {
        double nr[4] = {0.0, 0.0, 0.0, 0.0}, dr = 0.0;
        if (pinned(BX[i]) && pinned(BY[i])) {
            const Taps t = taps_of(BX[i], BY[i], h, w);
            for (int j = 0; j < 4; ++j) {
                if (t.row[j] < 0 || t.row[j] > h + 1 || t.col[j] < 0 || t.col[j] > w + 1) return fail("tap outside the padded grid", t.row[j], t.col[j]);
                if (!(t.prox[j] >= 0.0 && t.prox[j] <= 1.0)) return fail("proximity weight outside [0, 1]", i, j);
                const long long tap = frame_index(t.row[j], t.col[j], h, w), cell = (long long)t.row[j] * (w + 2) + t.col[j];
                if (tap < -1 || tap >= n) return fail("tap index out of range", i, tap);
                const double m = (tap >= 0 && mask2[tap] != 0.0) ? 1.0 : 0.0;
                if (m != mask_padded[cell]) return fail("tap mask differs from the padded copy", i, j);
                for (int ch = 0; ch < c; ++ch) {
                    const double v = tap >= 0 ? frame2[tap * c + ch] : 0.0;
                    if (!same_bits(v, frame_padded[cell * c + ch])) return fail("tap value differs from the padded copy", i, j);
                    const double term = t.prox[j] * v * m;
                    nr[ch] = j == 0 ? term : nr[ch] + term;
                }
                dr = j == 0 ? t.prox[j] * m : dr + t.prox[j] * m;
            }
        }
        for (int ch = 0; ch < c; ++ch) back[i * c + ch] = dr > 0.0 ? nr[ch] / dr : 0.0;
        back_dr[i] = dr;
    }

    // ---- to_image: clip, half to even, NaN -> 0
    const double image_in[10] = {-3.0, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, 127.49999999, NAN, -0.0};
    const int image_out[10] = {0, 0, 2, 2, 254, 255, 255, 127, 0, 0};
    for (int k = 0; k < 10; ++k)
        if (to_image(image_in[k]) != image_out[k]) return fail("to_image", k, to_image(image_in[k]));

    f = std::fopen(argv[5], "wb");
    if (!f || std::fwrite(out, sizeof(double), total_out, f) != (size_t)total_out) return fail("cannot write the output", 0, 0);
    std::fclose(f);
    delete[] in; delete[] out; delete[] keys; delete[] starts; delete[] order; delete[] cursor; delete[] sum_all; delete[] ws_all;
    delete[] frame_padded; delete[] mask_padded;
    std::printf("warp_cells_test: OK\n");
    return 0;
}
