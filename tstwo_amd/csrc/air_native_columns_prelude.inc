R"AIRN(
// The helpers of column kernels alone (csrc/air_codegen.h appends this text behind the prelude above for a STORE program; the
// text of an ACC program does not contain it).  They restate what k_air_columns of air.hip uses: the neighbour on the trace
// domain itself and the store of a lane's W rows.
namespace airn {

// the third kernel argument, as csrc/air_native.h (ColumnsArgs) fills it
struct ColumnsArgs { u32 n_rows, log, stride; };   // stride: lanes of the whole grid

// The output table: the second kernel argument, by value directly behind the input table (at most 64 outputs, so `ext` is null
// unless a caller of another shape ever fills it).
AIRN_DEV k64 out_table(const ColPtrs &o) {
    typedef const char AIRN_CONST *kbytes;
    return o.ext ? (k64)(u64)o.ext : (k64)((kbytes)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(ColPtrs));
}
AIRN_DEV u32 *out_at(k64 otab, u32 k) { return (u32 *)otab[k]; }

// trace_neighbour_row of air.hip (the eval_log == trace_log case of offset_bit_reversed_circle_domain_index): in coset order the
// neighbour of row k is row (k + off) mod 2^log; coset row k = 2 j + odd sits at position 2 t + odd with t = rev(j) for even k
// and ~rev(j) for odd k, rev over log - 1 bits.
AIRN_DEV u32 rev_bits(u32 x, u32 bits) { return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0; }
AIRN_DEV u32 trace_neighbour_row(u32 r, u32 log, int off) {
    const u32 L = log - 1, mask = (1u << L) - 1;
    const u32 odd = r & 1, t = r >> 1;
    const u32 k = 2 * rev_bits(odd ? ~t & mask : t, L) + odd;
    const u32 k2 = (k + (u32)off) & ((1u << log) - 1);
    const u32 odd2 = k2 & 1, t2 = rev_bits(k2 >> 1, L);
    return 2 * (odd2 ? ~t2 & mask : t2) + odd2;
}
template <int W> AIRN_DEV Rows<W> trace_neighbour_rows(u32 row, u32 log, int off) {
    Rows<W> r;
#pragma unroll
    for (int e = 0; e < W; e++) r.v[e] = trace_neighbour_row(row + e, log, off);
    return r;
}

// rows [row, row + W) of one output column: one 16-byte store per lane at W = 4, one word at W = 1
template <int W> AIRN_DEV void store_rows(u32 *col, u32 row, const Rows<W> &v) {
    if constexpr (W == 4) {
        u32x4_t x;
        x.x = v.v[0]; x.y = v.v[1]; x.z = v.v[2]; x.w = v.v[3];
        gstore4(col, row, x);
    } else {
        gstore1(col, row, v.v[0]);
    }
}

}  // namespace airn
)AIRN"
