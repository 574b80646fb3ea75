// Host-only half of the renderer (render_check.cpp): the font, the refusals of pa_render, the glyph resolution of a mark list.
#pragma once
#include "render_marks.h"

#include <cstddef>
#include <string>

namespace padel {

// rows[j] bit i = column i (0 = leftmost) of row j (0 = top); 1 for a code outside the font
int glyph_rows(int code, uint8_t rows[kGlyphH]);
// the list as render_marks.h reads it: glyph marks carry their 35 font bits in x1 / y1 (the list has passed render_validate)
void render_resolve_marks(const pa_mark* in, pa_mark* out, size_t count);
// every refusal of pa_render that needs no device pointer.  *dst_span = bytes of dst the kernel may write
int render_validate(int n, int h, int w, const pa_mark* marks, const int32_t* first, int out, const pa_yuv_desc* geom, const pa_yuv_enc* enc,
                    size_t* dst_span, std::string& err);
// the same for pa_render_scaled: h x w is the source, geom and *dst_span describe the (h / scale) x (w / scale) output;
// dst_is_src: the caller's dst is its src.  scale 1 is render_validate
int render_scaled_validate(int n, int h, int w, const pa_mark* marks, const int32_t* first, int scale, int out, const pa_yuv_desc* geom,
                           const pa_yuv_enc* enc, int dst_is_src, size_t* dst_span, std::string& err);

}  // namespace padel
