// csrc/conv_dispatch.h compiled on its own by the host compiler (no HIP): answers the id queries of tests/test_conv_dispatch_cpu.py
// from the decision functions directly, with `recording` as the plain argument it is there.
// stdin: one query per line, "<function> <recording 0|1> <arguments ...>"; stdout: one id per line.
#include "../../ransac-flow_amd/csrc/conv_dispatch.h"
#include <stdio.h>
#include <string.h>

int main() {
    const ConvKnobs& k = conv_knobs();
    char fn[64];
    int rec;
    while (scanf("%63s %d", fn, &rec) == 2) {
        int a[9] = {0}, n = !strcmp(fn, "rfx_conv2d_kernel_id") ? 9 : (!strcmp(fn, "rfx_conv3x3_kernel_id") ? 6 : 4);
        for (int i = 0; i < n; ++i)
            if (scanf("%d", &a[i]) != 1) return 2;
        int id;
        if (n == 9) id = conv_decide(k, {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]}, true, 0, true, rec != 0).id();
        else if (n == 6) id = conv_decide(k, {a[0], a[1], a[2], 3, 3, 1, 1, a[3], a[4]}, true, a[5], true, rec != 0).id();
        else if (!strcmp(fn, "rfx_conv2d_tile_variant")) id = conv_tile_variant(k, a[0], a[1], a[2], a[3]);
        else if (!strcmp(fn, "rfx_conv3x3_conv1x1_kernel_id")) id = conv_decide_tail(k, a[0], a[1], a[2], a[3], rec != 0).id();
        else return 3;
        printf("%d\n", id);
    }
    return 0;
}
