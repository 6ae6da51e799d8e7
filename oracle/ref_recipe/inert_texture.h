/* Force-included (-include) in front of the reference's bilateral file only.  That file keeps one dead entry point,
 * filter_bilateral_1_tex, written against the texture-reference API, which ROCm no longer offers on the device.  These
 * stand-ins let the file compile with its text untouched: the texture object is an empty type, a fetch yields 0 and
 * bind / unbind do nothing.  filter_bilateral_1_tex therefore returns nonsense and is never called; the live
 * filter_bilateral_1 / d_filter_bilateral_1 next to it use none of this. */
#pragma once
#include <hip/hip_runtime.h>
template <class T, int Dim, int Mode> struct stm_inert_texture {};
#define texture stm_inert_texture
#define tex1Dfetch(t, i) (0.0f)
#define hipBindTexture(...) (hipSuccess)
#define hipUnbindTexture(...) (hipSuccess)
