/*
 * line_offset_main.cpp -- p4_line_offset (rgbd_odometry_amd/csrc/dvo_palette.h), the byte offset the fused kernel gathers a pixel's rank
 * words at, against the layout's own definition p4_slot, as a stand-alone program: tests/test_line_offset_cpu.py builds it plainly and
 * under the address and undefined-behaviour sanitizers.
 *
 *   line_offset_main
 *
 * Every pixel of every level size with rows in 1..64 and {120, 240, 480, 1080, 3072}, cols in 1..40 and {160, 320, 640, 1920, 4096}:
 *     128 + p4_line_offset(yy, xx, tpc * 128 - 128)  ==  4 * p4_slot(yy / 6, yy - 6 * (yy / 6), xx, tpc),      tpc = p4_tiles_per_col(rows)
 * -- the word ABOVE the pixel (stored row yy - 6 ty; the pixel's own is the next), where the 12-byte gather starts -- and the same with
 * the lead the kernel adds (its base pointer sits that far short of the first real line).  Every offset with its 12 bytes lies inside
 * the image (p4_count).  Prints "ok <pixels checked>" and exits 0, or the first failure and exits 1.
 */
#include "dvo_palette.h"

#include <cstdio>
#include <vector>

int main() {
    using namespace dvo;
    std::vector<int> rows_list, cols_list;
    for (int r = 1; r <= 64; r++) rows_list.push_back(r);
    for (int r : {120, 240, 480, 1080, 3072}) rows_list.push_back(r);
    for (int c = 1; c <= 40; c++) cols_list.push_back(c);
    for (int c : {160, 320, 640, 1920, 4096}) cols_list.push_back(c);
    unsigned long long n = 0;
    for (int rows : rows_list)
        for (int cols : cols_list) {
            const int tpc = p4_tiles_per_col(rows);
            const unsigned rest = (unsigned)tpc * 128u - 128u;
            const size_t bytes = p4_count(rows, cols) * 4u;
            for (int xx = 0; xx < cols; xx++)
                for (int yy = 0; yy < rows; yy++) {
                    const int ty = yy / 6;
                    const size_t want = 4u * p4_slot(ty, yy - 6 * ty, xx, tpc);
                    const size_t got = 128u + (size_t)p4_line_offset(yy, xx, rest);
                    const size_t got_lead = 64u + (size_t)p4_line_offset<64u>(yy, xx, rest);
                    if (got != want || got_lead != want || want < 128u || want + 12u > bytes) {
                        std::printf("FAILED at rows=%d cols=%d yy=%d xx=%d: offset %zu, with the lead %zu, p4_slot says %zu, image of %zu bytes\n",
                                    rows, cols, yy, xx, got, got_lead, want, bytes);
                        return 1;
                    }
                    n++;
                }
        }
    std::printf("ok %llu\n", n);
    return 0;
}
