/* orbx_dev_pyr.h - one more test hook of the DEVELOPER build (see orbx_dev.h; the product library does not export it): the pyramid
 * level kernel's records.  It has a header of its own because the set of hooks orbx_dev.h declares is pinned by tests/test_abi_cpu.py. */
#ifndef ORBX_DEV_PYR_H
#define ORBX_DEV_PYR_H
#include "orbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The records k_pyr_level's waves read instead of deriving their set-up (csrc/orbx_size_plan.h: plan_pyr_records).
 * h == NULL: what the size decides, by itself - arguments as for orbx_debug_size_plan, no HIP call, no handle, works without a GPU; a size
 * ensure_plan would refuse returns its status.  h != NULL: the records of the handle's planned size as its DEVICE buffers hold them (the
 * other size arguments are ignored; ORBX_ERR_ARG before the handle's first call).
 *   cols    the first min(cols_cap, colWords) words of the column records: 4 words per (level >= 1, lane slot) = A, oa | ob << 8 |
 *           storeValid << 16, aa, ab; a level has nxc * 64 slots from record colOff
 *   bands   the first min(bands_cap, bandWords) words of the band records.  A record of the form with RW output rows per wave is
 *           8 + SR words (RW = 8: SR = 12, RW = 16: SR = 22): rf, mask, lastk, nrow, regular, byte offset of column -1 of the band's
 *           first row in the padded level, byte offset of source row rf from the padded row of source row 0, 0, then for k < SR
 *           b0 << 12 | b1 of the output row due after source row rf + k (0: none).  An irregular band (row-by-row path) has regular = 0
 *           and only rf, nrow and the row offset set.  64 zero words follow the last record (a wave loads 64 words from its record's start).
 *   index   (ORBX_DEBUG_PYR_RECORDS_INTS int32): colWords, bandWords, nxc[16], colOff[16], nbands[2][16] ([0] RW = 8, [1] RW = 16),
 *           bandOff[2][16] (first WORD of the level's band records of that form, -1: not built - levels 0 and, above scale factor 1.25,
 *           the 16-row form) */
#define ORBX_DEBUG_PYR_RECORDS_INTS 98
int orbx_debug_pyr_records(orbx_extractor_t *h, int nfeatures, float scale_factor, int nlevels, int w, int hgt, uint32_t *cols, int cols_cap,
                           uint32_t *bands, int bands_cap, int32_t *index, int n_index);

#ifdef __cplusplus
}
#endif
#endif
