// The route of the dense convolution's weight gradient (lsnet_amd/csrc/conv_wgrad_route.h) on the host, without a GPU: one line
// per case, "<name>: <route> ok" or "... MISMATCH, expected <route>", and a non-zero exit status when a case misses its row.
// tests/test_conv_wgrad_route_host.py builds this with g++ under the address and undefined-behaviour sanitizers.
// Unless a case says otherwise: six products per product, aligned pointers, the debug bit clear, padding k / 2.
#include <stdio.h>

#include "conv_wgrad_route.h"

static const char *NAMES[] = {"DENSE_MM", "PATCH", "PATCH_JOBS", "GENERAL"};

struct Map {
    int B, H, W;
};

static ConvWgradShape shape(int k, int stride, int dil, int C, int Co, int n, const Map *maps)
{
    ConvWgradShape s = {};
    const int pad = dil * (k / 2);
    s.n = n;
    for (int i = 0; i < n; ++i) {
        ConvWgradLevel &L = s.lv[i];
        L.B = maps[i].B, L.H = maps[i].H, L.W = maps[i].W;
        L.Ho = (L.H + 2 * pad - (dil * (k - 1) + 1)) / stride + 1, L.Wo = (L.W + 2 * pad - (dil * (k - 1) + 1)) / stride + 1;
        L.P = L.B * L.Ho * L.Wo;
    }
    s.C = C, s.Co = Co, s.kh = s.kw = k, s.stride = stride, s.dil = dil;
    s.aligned16 = true, s.np = 6, s.npl = 3, s.general_gemms = false, s.fold_jobs = 0;
    return s;
}
static ConvWgradShape shape(int k, int stride, int dil, int C, int Co, int B, int H, int W)
{
    const Map m = {B, H, W};
    return shape(k, stride, dil, C, Co, 1, &m);
}

static int g_bad = 0;
static void expect(const char *name, const ConvWgradShape &s, ConvWgradRoute want)
{
    const ConvWgradRoute got = conv_wgrad_route(s);
    if (got == want) {
        printf("%s: %s ok\n", name, NAMES[got]);
    } else {
        printf("%s: %s MISMATCH, expected %s\n", name, NAMES[got], NAMES[want]);
        ++g_bad;
    }
}

int main()
{
    ConvWgradShape s = shape(3, 1, 1, 256, 256, 2, 50, 84);
    expect("3x3 s1 256->256 2x50x84", s, CW_DENSE_MM);
    s.np = 0, s.npl = 0;
    expect("3x3 s1 256->256 2x50x84 exact mode", s, CW_PATCH);
    s = shape(3, 1, 1, 256, 256, 2, 50, 84), s.general_gemms = true;
    expect("3x3 s1 256->256 2x50x84 debug bit", s, CW_PATCH);
    s = shape(3, 1, 1, 256, 256, 2, 50, 84), s.aligned16 = false;
    expect("3x3 s1 256->256 2x50x84 pointer at offset 8", s, CW_PATCH);
    const Map two[2] = {{2, 50, 84}, {2, 50, 84}};
    s = shape(3, 1, 1, 256, 256, 2, two), s.fold_jobs = 2;
    expect("3x3 s1 256->256 2x50x84 two fold jobs", s, CW_PATCH_JOBS);
    expect("3x3 s1 64->256 1x64x64 (4096 px)", shape(3, 1, 1, 64, 256, 1, 64, 64), CW_DENSE_MM);
    expect("3x3 s1 64->256 1x63x65 (4095 px)", shape(3, 1, 1, 64, 256, 1, 63, 65), CW_PATCH);
    expect("3x3 s2 256->256 2x100x168", shape(3, 2, 1, 256, 256, 2, 100, 168), CW_DENSE_MM);
    expect("3x3 s2 128->128 2x22x18", shape(3, 2, 1, 128, 128, 2, 22, 18), CW_GENERAL);
    expect("3x3 s1 d2 64->64 2x22x18", shape(3, 1, 2, 64, 64, 2, 22, 18), CW_GENERAL);
    expect("7x7 s2 3->64 2x64x96", shape(7, 2, 1, 3, 64, 2, 64, 96), CW_GENERAL);
    s = shape(3, 1, 1, 256, 27, 2, 100, 168);
    expect("3x3 s1 256->27 2x100x168", s, CW_PATCH);
    s.np = 1, s.npl = 1;
    expect("3x3 s1 256->27 2x100x168 one product", s, CW_GENERAL);
    expect("3x3 s1 64->34 2x22x18", shape(3, 1, 1, 64, 34, 2, 22, 18), CW_GENERAL);
    expect("1x1 s1 256->27 2x22x18", shape(1, 1, 1, 256, 27, 2, 22, 18), CW_GENERAL);
    expect("1x1 s1 1024->512 1x50x48", shape(1, 1, 1, 1024, 512, 1, 50, 48), CW_DENSE_MM);
    expect("1x1 s1 1024->512 1x23x89 (2047 px)", shape(1, 1, 1, 1024, 512, 1, 23, 89), CW_PATCH);
    expect("1x1 s2 512->256 2x80x84", shape(1, 2, 1, 512, 256, 2, 80, 84), CW_DENSE_MM);
    expect("1x1 s1 1024->256 2x50x84", shape(1, 1, 1, 1024, 256, 2, 50, 84), CW_PATCH);
    expect("1x1 s1 128->512 2x100x168", shape(1, 1, 1, 128, 512, 2, 100, 168), CW_PATCH);
    expect("1x1 s2 1024->2048 2x50x84", shape(1, 2, 1, 1024, 2048, 2, 50, 84), CW_DENSE_MM);
    const Map head[5] = {{2, 100, 168}, {2, 50, 84}, {2, 25, 42}, {2, 13, 21}, {2, 7, 11}};
    expect("3x3 s1 256->256 five head levels", shape(3, 1, 1, 256, 256, 5, head), CW_DENSE_MM);
    expect("3x3 s1 256->256 2x1100x1100 (bytes >= 2^31)", shape(3, 1, 1, 256, 256, 2, 1100, 1100), CW_GENERAL);
    const Map two_s2[2] = {{2, 22, 18}, {2, 22, 18}};
    s = shape(3, 2, 1, 128, 128, 2, two_s2), s.fold_jobs = 2;
    expect("3x3 s2 128->128 two fold jobs: no shared launch", s, CW_GENERAL);
    s = shape(3, 2, 1, 128, 128, 2, 22, 18), s.fold_jobs = 1;
    expect("3x3 s2 128->128 each of the two jobs", s, CW_GENERAL);
    return g_bad ? 1 : 0;
}
