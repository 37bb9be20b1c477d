/*
 * acm_fir_layout.h - the device-free half of acm_batch_decode_windows_overlay_fir (acm_batch_windows.cpp): whether the responses and
 * the windows' numbers are ones the call takes, which windows are filtered, the taps of the responses they name as the kernel
 * (acm_dense_fir.hip) reads them, and where all of it sits behind the overlay call's tables.  Internal.  Neither this header nor
 * acm_fir_layout.cpp knows a device (tests/test_dense_fir.py).
 *
 * The arena trick: the source arena of the overlay call grows from nwin to nwin + nfilt rows, and F of the i-th filtered window is
 * row nwin + i.  acm_fir_remap rewrites the overlay layout - the row table that is uploaded, the list of rows to sum, the number of
 * arena rows - so that slot nwin + i stands wherever a filtered window k stood; the energy, gain and combine kernels then run
 * unchanged, and an unfiltered row is never copied.
 */
#ifndef ACM_FIR_LAYOUT_H
#define ACM_FIR_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "acm_device.h"
#include "acm_overlay_layout.h"

#define ACM_FIR_MAX_TAPS 32768u                 /* of one response */
#define ACM_FIR_MAX_L1 65535u                   /* sum |h[t]|: then |acc| <= 65535 * 32768 < 2^31 */
#define ACM_FIR_MAX_SHIFT 30u
#define ACM_FIR_MAX_RESPONSES 65536u
#define ACM_FIR_MAX_CALL_TAPS (1u << 22)        /* of the responses some window names, together */

namespace acmbatch {

struct FirLayout {
	size_t nwin = 0;
	std::vector<AcmFirRow> rows;            /* one per filtered window, ascending by window */
	std::vector<uint32_t> slot;             /* per window: the arena row the rest of the call reads - k, or nwin + i */
	std::vector<int16_t> taps;              /* the named responses, each once: reversed, zero-padded to whole tap blocks */
	size_t nfilt() const { return rows.size(); }
	/* the tables travel behind the overlay's in the H_JOBS / D_JOBS arenas, from `base` (a multiple of 64) on: taps, then rows */
	size_t taps_bytes() const { return taps.size() * sizeof(int16_t); }     /* a multiple of 128 */
	size_t rows_off() const { return taps_bytes(); }
	size_t table_bytes() const { return rows_off() + rows.size() * sizeof(AcmFirRow); }
};

/* ACMHIP_OK, or ACMHIP_ERR_ARG for what include/acm_hip.h refuses - then nothing of `out` is to be used.  fir == NULL, nresp == 0 or
 * every entry ACM_FIR_NONE: ACMHIP_OK and no filtered window */
int acm_fir_prepare(const acm_fir_opts *fir, size_t nwin, FirLayout *out);

/* the overlay layout of the same call seen through the filter: filtered windows named by their F rows, the arena that many rows longer */
void acm_fir_remap(const FirLayout &F, OverlayLayout *O);

} // namespace acmbatch

extern "C" {
typedef void (*acmk_fir_layout_visit_fn)(void *ctx, const char *name, const void *data, size_t elem_bytes, size_t count);
/* The layout shown to a visitor (tests): acm_overlay_prepare, acm_fir_prepare and acm_fir_remap over one call's arguments.  A refused
 * call visits "totals" alone.  Tables: "fir_rows" (uint64, 6 per filtered window: src, dst, taps_off, nblk, lead as two's complement,
 * shift), "slot" (uint64, 1 per window), "taps" (int16, as uploaded), "rows" (uint64, 5 per output row: a, b, vol, snr, gain as
 * uploaded), "marked" (uint64), "totals" (uint64): the return code, nfilt, taps_bytes, rows_off, table_bytes, the overlay's nsrc,
 * src_arena_words, energy_bytes and table_bytes, the tap block */
int acmk_fir_layout_visit(const acm_overlay_row *rows, size_t nrows, size_t nwin, uint64_t row_words, uint64_t d_pcm_words, const acm_fir_opts *fir,
			  acmk_fir_layout_visit_fn visit, void *ctx);
}

#endif
