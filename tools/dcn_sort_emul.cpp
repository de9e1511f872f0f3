// Sequential emulation of the anchor-list sort of the deformable backward (lsnet_amd/csrc/dcn_gather_kernels.h,
// dcn_list_*_kernel) on the arithmetic those kernels share with it (lsnet_amd/csrc/dcn_sort_plan.h): the same blocks, waves,
// rows and lanes, the same histograms, scans and position formula, every array sized exactly as the library sizes it.  Each
// case is compared with std::stable_sort.  Meant to be built with -fsanitize=address,undefined: a scatter position outside
// [0, nsamples) is a heap overflow here instead of a fault on a GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lsnet_amd/csrc tools/dcn_sort_emul.cpp -o dcn_sort_emul
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "dcn_sort_plan.h"

struct Pair {
    int key, s;
};

// histogram kernel: one workgroup per block, digit-major output; every (digit, block) cell is written
static void emul_hist(const std::vector<Pair> &in, int pass, int db, int nblocks, std::vector<int> &hist)
{
    const int n = (int)in.size(), ndig = 1 << db;
    for (int blk = 0; blk < nblocks; ++blk) {
        std::vector<int> h(ndig, 0);
        for (int i = blk * DS_BLOCK; i < std::min(n, (blk + 1) * DS_BLOCK); ++i) ++h[ds_digit(in[i].key, pass, db)];
        for (int d = 0; d < ndig; ++d) hist[ds_hist_at(d, blk, nblocks)] = h[d];
    }
}

// scan kernel: one workgroup per digit row, exclusive in place; the row's total behind the histogram
static void emul_scan(std::vector<int> &hist, int db, int nblocks)
{
    const int ndig = 1 << db;
    for (int d = 0; d < ndig; ++d) {
        int carry = 0;
        for (int b = 0; b < nblocks; ++b) {
            const int v = hist[ds_hist_at(d, b, nblocks)];
            hist[ds_hist_at(d, b, nblocks)] = carry;
            carry += v;
        }
        hist[ds_hist_at(ndig, 0, nblocks) + d] = carry;
    }
}

// scatter kernel
static void emul_scatter(const std::vector<Pair> &in, std::vector<Pair> &out, int pass, int db, int nblocks, const std::vector<int> &hist)
{
    const int n = (int)in.size(), ndig = 1 << db;
    const int *tot = hist.data() + ds_hist_at(ndig, 0, nblocks);
    for (int blk = 0; blk < nblocks; ++blk) {
        std::vector<int> gbase(ndig);
        std::vector<std::vector<int>> cnt(DS_WAVES, std::vector<int>(ndig, 0));
        int run = 0;
        for (int d = 0; d < ndig; ++d) gbase[d] = run + hist[ds_hist_at(d, blk, nblocks)], run += tot[d];
        std::vector<int> local(DS_BLOCK, 0);   // earlier rows + lower lanes, per element of the block
        for (int w = 0; w < DS_WAVES; ++w)
            for (int r = 0; r < DS_ROWS; ++r) {
                int prior[64], rank[64], rowcnt[64];
                for (int lane = 0; lane < 64; ++lane) {   // all lanes read the counts, then the leaders write
                    const int i = ds_elem(blk, w, r, lane);
                    prior[lane] = rank[lane] = rowcnt[lane] = 0;
                    if (i >= n) continue;
                    const int d = ds_digit(in[i].key, pass, db);
                    prior[lane] = cnt[w][d];
                    for (int l2 = 0; l2 < 64; ++l2) {   // the ballots' mask of the lanes with this digit
                        const int j = ds_elem(blk, w, r, l2);
                        if (j < n && ds_digit(in[j].key, pass, db) == d) ++rowcnt[lane], rank[lane] += l2 < lane;
                    }
                }
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = ds_elem(blk, w, r, lane);
                    if (i >= n) continue;
                    local[i - blk * DS_BLOCK] = prior[lane] + rank[lane];
                    if (rank[lane] == 0) cnt[w][ds_digit(in[i].key, pass, db)] = prior[lane] + rowcnt[lane];
                }
            }
        for (int d = 0; d < ndig; ++d) {   // counts -> the digit's count in earlier waves
            int before = 0;
            for (int w = 0; w < DS_WAVES; ++w) {
                const int c = cnt[w][d];
                cnt[w][d] = before;
                before += c;
            }
        }
        for (int w = 0; w < DS_WAVES; ++w)
            for (int r = 0; r < DS_ROWS; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = ds_elem(blk, w, r, lane);
                    if (i >= n) continue;
                    const int d = ds_digit(in[i].key, pass, db);
                    const int pos = ds_position(gbase[d], cnt[w][d], local[i - blk * DS_BLOCK]);
                    out[pos] = in[i];   // (the device guards pos < n; here an overflow must be seen)
                }
    }
}

static int run_case(const char *name, int nanchors, const std::vector<int> &keys)
{
    const int n = (int)keys.size();
    const int db = ds_digit_bits(nanchors), passes = ds_passes(nanchors), nblocks = ds_blocks(n);
    if (db > DS_MAX_DIGIT_BITS || passes * db < ds_key_bits(nanchors)) {
        printf("%s: digit plan does not cover the key (%d passes x %d bits, key %d bits)\n", name, passes, db, ds_key_bits(nanchors));
        return 1;
    }
    std::vector<Pair> a(n), b(n);
    for (int s = 0; s < n; ++s) a[s] = {keys[s], s};
    std::vector<int> hist(ds_hist_ints(n, nanchors), -1);
    for (int p = 0; p < passes; ++p) {
        emul_hist(a, p, db, nblocks, hist);
        emul_scan(hist, db, nblocks);
        std::fill(b.begin(), b.end(), Pair{-1, -1});
        emul_scatter(a, b, p, db, nblocks, hist);
        a.swap(b);
    }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return keys[x] < keys[y]; });
    for (int i = 0; i < n; ++i)
        if (a[i].s != order[i] || a[i].key != keys[order[i]]) {
            printf("%s: position %d holds sample %d (key %d), expected sample %d (key %d)\n", name, i, a[i].s, a[i].key, order[i],
                   keys[order[i]]);
            return 1;
        }
    // starts: lower bound of every anchor in the sorted keys; start[nanchors] = listed samples
    int listed = 0;
    for (int s = 0; s < n; ++s) listed += keys[s] != nanchors;
    for (int an : {0, nanchors / 2, nanchors - 1, nanchors}) {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (a[mid].key < an) lo = mid + 1; else hi = mid;
        }
        int ref = 0;
        for (int s = 0; s < n; ++s) ref += keys[s] < an;
        if (lo != ref || (an == nanchors && lo != listed)) {
            printf("%s: start[%d] = %d, expected %d\n", name, an, lo, ref);
            return 1;
        }
    }
    printf("%-28s ok: %8d samples, %10d anchors, %d passes x %2d bits, %d blocks\n", name, n, nanchors, passes, db, nblocks);
    return 0;
}

int main()
{
    std::mt19937 rng(12345);
    int bad = 0;
    auto uniform = [&](int n, int nanchors, double none) {
        std::vector<int> k(n);
        std::uniform_int_distribution<int> u(0, nanchors - 1);
        std::uniform_real_distribution<double> f(0.0, 1.0);
        for (int &v : k) v = f(rng) < none ? nanchors : u(rng);
        return k;
    };
    // random offsets: a fifth of the samples outside the map; ragged last block and last wave
    bad += run_case("random 13x21", 2 * 14 * 22, uniform(2 * 13 * 21 * 9, 2 * 14 * 22, 0.2));
    bad += run_case("random tower-like", 45852, uniform(44800 * 9 / 4 + 777, 45852, 0.1));
    // every sample on one anchor: one list over eight blocks; and on the first / last anchor
    bad += run_case("converging", 2 * 11 * 11, std::vector<int>(14400, 137));
    bad += run_case("converging two levels", 2 * 11 * 11, std::vector<int>(2 * (1600 + 400) * 9, 60));
    bad += run_case("all on anchor 0", 65536, std::vector<int>(5000, 0));
    bad += run_case("all on the last anchor", 65536, std::vector<int>(5000, 65535));
    // no sample on any list
    bad += run_case("all outside", 2 * 41 * 41, std::vector<int>(2 * 1600 * 9, 2 * 41 * 41));
    // digit boundaries: the sentinel needs a 17th bit; 66 248 anchors
    bad += run_case("65536 anchors", 65536, uniform(255 * 255 * 9 / 8, 65536, 0.3));
    bad += run_case("66248 anchors", 66248, uniform(2 * 181 * 181 * 9 / 8, 66248, 0.3));
    {   // keys at both ends of every digit
        std::vector<int> k;
        for (int rep = 0; rep < 700; ++rep)
            for (int v : {0, 1, 255, 256, 257, 511, 512, 65279, 65280, 65535, 65536}) k.push_back(v);
        std::shuffle(k.begin(), k.end(), rng);
        bad += run_case("digit edges", 65536, k);
    }
    // tiny launches
    bad += run_case("3x3 map", 16, uniform(81, 16, 0.3));
    bad += run_case("one sample", 4, std::vector<int>(1, 3));
    bad += run_case("one block exactly", 300, uniform(DS_BLOCK, 300, 0.1));
    bad += run_case("one block and one", 300, uniform(DS_BLOCK + 1, 300, 0.1));
    // widest two-pass digits (11 + 11 bits), three passes, the largest anchor count the plan admits
    bad += run_case("2^22 - 1 anchors", (1 << 22) - 1, uniform(30000, (1 << 22) - 1, 0.1));
    bad += run_case("2^22 anchors: three passes", 1 << 22, uniform(30000, 1 << 22, 0.1));
    bad += run_case("2^30 - 1 anchors", (1 << 30) - 1, uniform(30000, (1 << 30) - 1, 0.1));
    if (bad) printf("%d case(s) FAILED\n", bad);
    return bad ? 1 : 0;
}
