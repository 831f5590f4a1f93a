// tests/rows_plan_dump.cpp -- compiled by tests/test_rows_plan.py with a plain C++ compiler: answers questions about csrc/pt_rows_plan.hpp, one
// per line of standard input, one line of output each:
//   halo I                         -> filter_halo_rows
//   fwin H R0 N I                  -> "row0 nrows" of filter_window
//   band W0 WN R0 N I i            -> "row0 nrows" of filter_band
//   uwin H F R0 N                  -> "row0 nrows" of upsample_low_window
//   fcheck H W0 WN R0 N I          -> the RowsVerdict code of filter_rows_check (0 ok, 1 empty, 2 outside the image, 3 window short)
//   ucheck H F R0 N L0 LN          -> the RowsVerdict code of upsample_rows_check
//   plan N (S0 SN D0 DN) x N       -> "<ExchangeVerdict code> <at> <copies> (src_ctx src_row dst_ctx dst_row nrows) x copies"
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pt_rows_plan.hpp"

static bool read(uint32_t* v, int n) {
    for (int i = 0; i < n; ++i)
        if (scanf("%" SCNu32, v + i) != 1) return false;
    return true;
}

int main() {
    char what[16];
    uint32_t v[8];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "halo")) {
            if (!read(v, 1)) return 1;
            printf("%" PRIu32 "\n", pt::filter_halo_rows(v[0]));
        } else if (!strcmp(what, "fwin")) {
            if (!read(v, 4)) return 1;
            const pt::RowRange r = pt::filter_window(v[0], v[1], v[2], v[3]);
            printf("%" PRIu32 " %" PRIu32 "\n", r.row0, r.nrows);
        } else if (!strcmp(what, "band")) {
            if (!read(v, 6)) return 1;
            const pt::RowRange r = pt::filter_band(v[0], v[1], v[2], v[3], v[4], v[5]);
            printf("%" PRIu32 " %" PRIu32 "\n", r.row0, r.nrows);
        } else if (!strcmp(what, "uwin")) {
            if (!read(v, 4)) return 1;
            const pt::RowRange r = pt::upsample_low_window(v[0], v[1], v[2], v[3]);
            printf("%" PRIu32 " %" PRIu32 "\n", r.row0, r.nrows);
        } else if (!strcmp(what, "fcheck")) {
            if (!read(v, 6)) return 1;
            printf("%d\n", (int)pt::filter_rows_check(v[0], v[1], v[2], v[3], v[4], v[5]));
        } else if (!strcmp(what, "ucheck")) {
            if (!read(v, 6)) return 1;
            printf("%d\n", (int)pt::upsample_rows_check(v[0], v[1], v[2], v[3], v[4], v[5]));
        } else if (!strcmp(what, "plan")) {
            if (!read(v, 1) || v[0] > 64u) return 1;
            const size_t n = v[0];
            std::vector<uint32_t> s0(n), sn(n), d0(n), dn(n);
            for (size_t i = 0; i < n; ++i)
                if (!read(&s0[i], 1) || !read(&sn[i], 1) || !read(&d0[i], 1) || !read(&dn[i], 1)) return 1;
            std::vector<pt::RowCopy> plan;
            size_t at = 0;
            const pt::ExchangeVerdict e = pt::exchange_plan(s0.data(), sn.data(), d0.data(), dn.data(), n, &plan, &at);
            printf("%d %zu %zu", (int)e, at, plan.size());
            for (const pt::RowCopy& c : plan) printf(" %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32, c.src_ctx, c.src_row, c.dst_ctx, c.dst_row, c.nrows);
            printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
