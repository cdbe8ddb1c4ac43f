// The marker flags' span in a batch's read-back staging (aruco3_amd/csrc/a3_readback.h, ReadbackShape::flags): off by default, and then
// every span and the end are what they are without the switch; on, one word per marker behind everything else -- of the guess when
// staged, of the whole list in the re-fetch.  A stand-alone program, built with the address and undefined-behaviour sanitizers by
// tests/test_inverted_abi.py.  tests/readback_layout.cpp holds every combination without flags to the parent's offsets.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../aruco3_amd/csrc/a3_readback.h"
using namespace a3;
#define CHECK(c) do { checks++; if (!(c)) { printf("FAILED %s (line %d) features %u n %u guess %u\n", #c, __LINE__, features, n, guess); return 1; } } while (0)
int main() {
    long checks = 0;
    for (unsigned features = 0; features < 64; features++)
        for (uint32_t n : {1u, 3u, 256u})
            for (uint32_t guess : {0u, 1u, 64u, 65u, 4096u}) {
                const ReadbackShape off{n, guess, n * 4u, 264, (features & 1) != 0, (features & 2) != 0, (features & 4) != 0, (features & 8) != 0,
                                        (features & 16) != 0, (features & 32) != 0};
                ReadbackShape on = off;
                on.flags = true;
                CHECK(!off.flags);
                for (int refetch = 0; refetch < 2; refetch++) {
                    const uint32_t total = 10u * guess + 7u, markers = refetch ? total : guess;
                    const Readback a = refetch ? refetch_layout(off, total) : readback_layout(off);
                    const Readback b = refetch ? refetch_layout(on, total) : readback_layout(on);
                    CHECK(a.flags.bytes == 0 && a.flags.off == a.end);
                    CHECK(b.flags.off == a.end && b.flags.bytes == (size_t)markers * 4 && b.end == a.end + (size_t)markers * 4);
                    CHECK(b.flags.off % 4 == 0);
                    CHECK(a.head.off == b.head.off && a.head.bytes == b.head.bytes && a.markers.off == b.markers.off && a.markers.bytes == b.markers.bytes);
                    CHECK(a.charuco_total.off == b.charuco_total.off && a.charuco.off == b.charuco.off && a.charuco.bytes == b.charuco.bytes);
                    for (int k = 0; k < kSideKinds; k++) CHECK(a.side[k].off == b.side[k].off && a.side[k].bytes == b.side[k].bytes);
                    CHECK(sides_on(off) == sides_on(on));
                    CHECK(pinned_bytes(b) >= b.end);
                }
            }
    printf("ok: %ld checks\n", checks);
    return 0;
}
