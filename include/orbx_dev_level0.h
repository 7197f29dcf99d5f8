/* orbx_dev_level0.h - one more test hook of the DEVELOPER build (see orbx_dev.h, which includes this file; the product library does not
 * export it): which input form an extraction call ran.  It has a header of its own because the set of hooks orbx_dev.h declares itself
 * is pinned by tests/test_abi_cpu.py. */
#ifndef ORBX_DEV_LEVEL0_H
#define ORBX_DEV_LEVEL0_H
#include "orbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The form the handle's last extraction call ran: 1 = level 0 was read in place from the caller's images
 * (orbx_extract_batch_device_padded and the pyramid it or its _prefetch companion built), 0 = level 0 was copied into the handle's
 * pyramid block (every other entry point, and the padded one when it falls back: level-wide blur of level 0, at most 4 images in
 * the call or in its smallest chunk, a developer knob that picks another pyramid form).  ORBX_ERR_ARG before the handle's first call.  Results never depend on the form. */
int orbx_debug_level0_in_place(const orbx_extractor_t *h);

#ifdef __cplusplus
}
#endif
#endif
