/*
 * acm_launch_caps.h - how much work ONE launch of the list-sliced and grid-capped kernels takes, and the test aid that lowers it
 * (acmhip_device_set_launch_caps, include/acm_hip.h).  Plain C, no device: the launchers, the setter and the tests read these
 * five numbers here and nowhere else.
 */
#ifndef ACM_LAUNCH_CAPS_H
#define ACM_LAUNCH_CAPS_H

#include <stdint.h>

#define ACM_CAP_LIST_SLICE    65535u        /* gridDim.y carries the stream index of acm_small, acm_sw_unpack / stage / prefix and acm_emit */
#define ACM_CAP_SMALL_GRID_X  4096u         /* acm_small strides over its stream from there on */
#define ACM_CAP_PARSE_SLICE   65535u        /* gridDim.y carries the job index of acm_parse_columns */
#define ACM_CAP_PARSE_GRID_X  2048u         /* ... which strides over its columns from there on */
#define ACM_CAP_DENSE_GRID    (1u << 20)    /* every dense kernel strides over its (row, sub-row, unit) items from there on */

typedef struct acmhip_launch_caps {   /* 0 in a field = the built-in value */
	uint32_t list_slice;     /* streams per launch of the list-sliced synthesis kernels (built-in 65535) */
	uint32_t small_grid_x;   /* workgroups along x of the level 0-4 register kernel (built-in 4096)     */
	uint32_t parse_slice;    /* jobs per launch of the column kernel (built-in 65535)                   */
	uint32_t parse_grid_x;   /* its workgroups along x (built-in 2048)                                   */
	uint32_t dense_grid;     /* workgroups of every dense kernel (built-in 2^20)                         */
} acmhip_launch_caps;

/* what a launcher does with a cap it is handed: 0 is the built-in value, and nothing raises one */
static inline uint32_t acm_cap_value(uint32_t cap, uint32_t builtin)
{
	return cap == 0 || cap > builtin ? builtin : cap;
}

#endif
