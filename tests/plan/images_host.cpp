/* The pure half of pc_images.h compiled for the host alone: what tests/test_image_plan_cpu.py checks.  Options cross the boundary
 * as an array in the order of the name list below, which the Python side reads from here. */
#include "pc_images.h"

#include <cstdint>

#define IMAGE_OPTS(X) X(plane_images) X(compact_images) X(compact_parts) X(slot_ids) X(blk_shift) X(run_parts) X(fetch_threads) \
	X(keep_pinned) X(dst_prepinned)
#define PLAN_FIELDS(X) X(layout) X(n_slots) X(elems) X(parts) X(fetch_parts) X(halves) X(blk_shift) X(blocks)

#define NAME(f) #f " "
#define COUNT(f) + 1
static_assert(sizeof(pc_image_opts) == (0 IMAGE_OPTS(COUNT))*sizeof(int), "IMAGE_OPTS lists every option of pc_image_opts");

extern "C" {

const char *images_opt_names(void) { return IMAGE_OPTS(NAME); }
const char *images_plan_field_names(void) { return PLAN_FIELDS(NAME); }
int images_n_fields(void) { return PC_N_FIELDS; }
int images_max_parts(void) { return PC_MAX_PARTS; }

void images_default_opts(int32_t *opts)
{
	const pc_image_opts o;
#define GET(f) *opts++ = o.f;
	IMAGE_OPTS(GET)
#undef GET
}

/* fields: PLAN_FIELDS; begin: PC_MAX_PARTS + 1 entries */
void images_plan(int64_t n_slots, int ne, int keep_images, const int32_t *opts, int64_t *fields, int64_t *begin)
{
	pc_image_opts o;
#define SET(f) o.f = *opts++;
	IMAGE_OPTS(SET)
#undef SET
	const pc_image_plan p = pc_plan_images(n_slots, ne, keep_images != 0, o);
#define GET(f) *fields++ = (int64_t)p.f;
	PLAN_FIELDS(GET)
#undef GET
	for (int k = 0; k <= PC_MAX_PARTS; k++) begin[k] = p.begin[k];
}

/* out: ss, fs, ws, base, w_base */
void images_layout(int layout, int64_t n_total, int64_t ne, int64_t lo, int64_t *out)
{
	const pc_image_layout l = pc_layout_of(layout, n_total, ne, lo);
	out[0] = l.ss; out[1] = l.fs; out[2] = l.ws; out[3] = (int64_t)l.base; out[4] = (int64_t)l.w_base;
}

void images_block_span(int64_t first, int64_t count, int64_t n_total, int blk_shift, int64_t b, int64_t e, int64_t *out)
{
	long long lo, hi;
	pc_block_span(first, count, n_total, blk_shift, b, e, lo, hi);
	out[0] = lo; out[1] = hi;
}

void images_planes(const pc_hip_images *d, void **out) { pc_image_planes(d, out); }

}
