// v3d_depth_math.h -- the depth-range arithmetic of libv3d_hip, written once.  Plain C11 for host and device, no HIP header:
// tests/test_depth_math_host.py compiles it with the oracle's gcc and holds it to the NumPy contracts bit for bit.  Every float
// step is one correctly rounded float32 operation in the reference's order (-ffp-contract=off; HIP's `/` is correctly rounded).
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>

#ifdef __HIPCC__
#define V3D_HD __host__ __device__
#else
#define V3D_HD
#endif

// order-preserving float <-> uint32 codec: a < b as floats iff f2ord(a) < f2ord(b) as unsigned (-0 sorts below +0), so an
// unsigned atomicMin / atomicMax reduces floats.  An empty {min, max} slot is {0xFFFFFFFF, 0}.
V3D_HD static inline uint32_t v3d_f2ord(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
V3D_HD static inline float v3d_ord2f(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// the fixed-point disparity d16 = rint(16 D), round half to even, as a float (NaN stays NaN, nothing saturates); valid iff >= 1
V3D_HD static inline float v3d_d16(float d) { return rintf(d * 16.0f); }

// the same fixed point as an integer (robust histogram, flicker; the statement tests/temporal_ref.py d16_of restates): 0 = invalid,
// else 1 .. 32767.  Validity is decided in float, before any conversion: valid iff 1 <= rint(16 D), which NaN, -inf, -0.0, a
// denormal and every D < 1/32 fail (D = 1/32 is a tie and goes to the even 0).  A valid sample above the range, +inf included,
// saturates to V3D_D16_MAX, so the value converted is always one an int holds.  The temporal filter's tap loop decides validity
// the same way and keeps (int)v3d_d16(D), unclamped, for a valid tap's value, with a stated domain: the clamp cost it 3 to 4 %
// ("Non-finite input").
#define V3D_D16_MAX 32767
V3D_HD static inline int v3d_d16_tap(float d)
{
    const float r = v3d_d16(d);
    return (int)(r >= (float)V3D_D16_MAX ? (float)V3D_D16_MAX : r >= 1.0f ? r : 0.0f);
}

// save_depth_map's ((d - lo) / (hi - lo) * 65535).astype(uint16) in float32; a flat or unordered range gives 0.  The clamp to
// [0, 65535] matters only for a d outside [lo, hi] (a filtered blend may round up to 1/32 outside its window's range); NaN -> 0
V3D_HD static inline uint16_t v3d_norm_u16(float d, float lo, float hi)
{
    if (!(hi > lo)) return 0;
    const float v = (d - lo) / (hi - lo) * 65535.0f;
    return (uint16_t)(v >= 65535.f ? 65535.f : v > 0.f ? v : 0.f);
}

// the 16-bit sample of the 4K PNG sink: round to nearest even (numpy.rint / torch.round), clamp to [0, 65535], NaN -> 0
V3D_HD static inline uint16_t v3d_rint_u16(float q)
{
    const float v = rintf(q);
    return (uint16_t)(v >= 65535.f ? 65535.f : v > 0.f ? v : 0.f);
}
