// Every row slab [p0, p1) of an instance of csrc/jk_m8.hip through m8_ranges: the split of the tiles over the workgroups
// and, beside it, M8Tables (where each workgroup's range starts: offset of its first tile, row of that tile), which
// m8_ranges itself compares with m8_tile_offset / m8_tri_row when it fills them.  Here: that comparison reports nothing,
// and what it does not look at -- the ranges are contiguous and cover the slab, the offsets rise with the workgroups and
// stay inside the packed slab, an entry of a workgroup without tiles is never out of range.  Built by
// tests/test_host_jk_m8_tables.py with the host sanitizers; links the library for the few symbols jk_m8.hip refers to.
#include "jk_m8.hip"

template <int NB>
int sweep() {
    using G = M8Geom<NB, m8_lp(NB)>;
    int nbad = 0;
    long ncase = 0;
    auto fail = [&](const char* what, int p0, int p1, long a, long b) {
        if (nbad++ < 8) printf("N=%d [%d,%d): %s (%ld, %ld)\n", G::N, p0, p1, what, a, b);
    };
    for (int p0 = 0; p0 < G::N; ++p0)
        for (int p1 = p0 + 1; p1 <= G::N; ++p1, ++ncase) {
            int wgs;
            const M8Tables* tb;
            const char* bad;
            const M8Ranges& rg = m8_ranges<G>(p0, p1 - p0, &wgs, &tb, &bad);
            if (bad != nullptr) {
                if (nbad++ < 8) printf("N=%d [%d,%d): %s\n", G::N, p0, p1, bad);
                continue;
            }
            const long ntiles = m4_tri(p1) - m4_tri(p0);
            const long units = (long)((nbx_jk_m8_packed_bytes(G::N, p0, p1) - 256) / (16 * sizeof(double)));
            if (rg.first[0] != 0 || rg.first[wgs] != ntiles) fail("cover", p0, p1, rg.first[0], rg.first[wgs]);
            long last_off = -1;
            for (int w = 0; w < wgs; ++w) {
                if (rg.first[w + 1] < rg.first[w]) fail("order", p0, p1, w, rg.first[w]);
                const int row = m8_byte(tb->pfirst, w);
                if (row >= G::N || tb->tile_off[w] < 0 || tb->tile_off[w] >= units) fail("range", p0, p1, w, tb->tile_off[w]);
                if (rg.first[w + 1] == rg.first[w]) continue;
                if (row < p0 || row >= p1) fail("row", p0, p1, w, row);
                if (tb->tile_off[w] <= last_off) fail("offsets rise", p0, p1, w, tb->tile_off[w]);
                last_off = tb->tile_off[w];
            }
        }
    printf("N=%d: %ld slabs, bad=%d\n", G::N, ncase, nbad);
    return nbad;
}

int main() {
    int bad = 0;
#define M8_CHECK_SWEEP(NB_) bad += sweep<NB_>();
    NBX_M8_SIZES(M8_CHECK_SWEEP)
    return bad != 0;
}
