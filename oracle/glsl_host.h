/*
 * glsl_host.h — the GLSL subset of the reference's on-path compute shaders, for a C++20 compiler.
 * TEST INFRASTRUCTURE ONLY. ref_shaders.cpp includes this header and then the reference's shader
 * texts, prepared by prepare_shader.py into oracle/_ref/gen/ (never committed), one namespace each.
 *
 * ======================================= THE NUMBER MODEL =======================================
 * A C++ compiler is not glslang. Every difference the shaders can notice is settled here, once.
 *
 * N1  Run-time scalars are wrapper classes, not C++'s own types. ref_shaders.cpp defines
 *         float -> glsl::Float     int -> glsl::Int<int32_t>     uint -> glsl::Int<uint32_t>
 *     for the shader texts only. A Float holds one IEEE binary32 and has no conversion to any
 *     C++ arithmetic type, so no C++ promotion to double can slip into a shader expression.
 *     The build uses -ffp-contract=off -fno-fast-math and no FMA target, as the oracle does.
 * N2  C++'s `double` plays the part of glslang's constant. glslang keeps a floating constant as a
 *     double, folds constant expressions in double and narrows once when the value becomes a
 *     32-bit OpConstant. A floating literal is a C++ double, an integer literal is a C++ int, and
 *     C++ folds their arithmetic in double: `1.0 / 4` is the double 0.25.
 *     `const float a = 0.3;` is a constant expression in GLSL, so it must stay a double:
 *     the preparation step writes `const auto a = glsl_const(0.3);`, and glsl_const() returns a
 *     double for a constant initialiser and a Float for a run-time one. With it
 *     img_smooth.comp:24-30 gives {0.1f, 0.25f, 0.3f, 0.25f, 0.1f}; float arithmetic would give
 *     0.099999994f. A const ARRAY indexed by a variable is a run-time load: its elements are
 *     Floats, each narrowed once from its folded initialiser.
 * N3  A constant that meets a run-time value is narrowed to binary32 FIRST and the operation is a
 *     binary32 operation: `currPixel / 0.1` divides by 0.1f (noise_hist.comp:31) and
 *     `maxCount * 0.05` is float(maxCount) * 0.05f (gradation_curve_generate.comp:88). This is what
 *     Float(double) and the Int-with-double operators below do. A run-time integer meeting a
 *     float operand is converted to binary32 as GLSL's implicit conversion does.
 *     Limit of the model: C++ cannot tell an int literal from the int RESULT of integer
 *     arithmetic, so `(i + 1) * (1.0 / 512)` (gradation_curve_debug_render.comp:100-115) multiplies
 *     in double. Both operands are exact there (small integer, power of two), so the double
 *     product narrowed once equals the binary32 product. No on-path shader has such a form with an
 *     inexact constant.
 *
 * N4  A vec4 stored to an rgba8 image is converted as Vulkan's UNORM rule says (spec "Conversion from floating-point to
 *     normalized fixed-point"): clamp to [0, 1], times 255, round to nearest: unorm8(). The two plot shaders store only
 *     0 and 1, which give the bytes 0 and 255 under any rounding.
 *
 * The remaining liberties are SURVEY §8 Q1..Q6, each ONE named function below:
 *   Q1  q1_in_bounds()        out-of-bounds imageLoad gives 0, imageStore / imageAtomicAdd is dropped
 *   Q2  (caller)              never-written texels read as 0: the callers hand in zeroed arrays
 *   Q3  clamp()               a real clamp; the shaders discard its result, so it does nothing
 *   Q4  q4_uvec4_to_r32f()    a uvec4 stored to an r32f image stores float(uint(value))
 *   Q5  q5_pow()              pow(x, 2) == x * x, pow(r, 5.0) == ((r*r)*(r*r))*r; no other exponent
 *   Q6  q6_float_to_int()     truncates, saturates outside int32 (what the oracle drops as an
 *       q6_float_to_uint()    index lands outside every image), NaN -> 0; to uint: negative and
 *                             NaN -> 0, saturates high
 * ================================================================================================
 */
#ifndef GLSL_HOST_H
#define GLSL_HOST_H

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <type_traits>

namespace glsl {

/* ---- Q rules ------------------------------------------------------------------------------- */
inline bool q1_in_bounds(int32_t x, int32_t y, int32_t w, int32_t h) { return x >= 0 && y >= 0 && x < w && y < h; }

inline int32_t q6_float_to_int(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return (int32_t)v;
}
inline uint32_t q6_float_to_uint(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}
inline float q4_uvec4_to_r32f(uint32_t component) { return (float)component; }
inline float q5_pow(float x, float y) {
    if (y == 2.0f) return x * x;
    if (y == 5.0f) return ((x * x) * (x * x)) * x;
    std::fprintf(stderr, "glsl_host: pow(x, %g) has no Q5 restatement\n", (double)y);
    std::abort();
}

/* ---- run-time scalars (N1) ------------------------------------------------------------------ */
template <class B> struct Int;

struct Float {
    float v;
    Float() = default;
    Float(float f) : v(f) {}
    Float(double constant) : v((float)constant) {}          /* N2/N3: narrowed once */
    Float(int i) : v((float)i) {}
    Float(unsigned u) : v((float)u) {}
    template <class B> Float(Int<B> i);
    friend Float operator+(Float a, Float b) { return Float(a.v + b.v); }
    friend Float operator-(Float a, Float b) { return Float(a.v - b.v); }
    friend Float operator*(Float a, Float b) { return Float(a.v * b.v); }
    friend Float operator/(Float a, Float b) { return Float(a.v / b.v); }
    friend Float operator-(Float a) { return Float(-a.v); }
    friend bool operator==(Float a, Float b) { return a.v == b.v; }
    friend bool operator!=(Float a, Float b) { return a.v != b.v; }
    friend bool operator<(Float a, Float b) { return a.v < b.v; }
    friend bool operator>(Float a, Float b) { return a.v > b.v; }
    friend bool operator<=(Float a, Float b) { return a.v <= b.v; }
    friend bool operator>=(Float a, Float b) { return a.v >= b.v; }
    Float& operator+=(Float b) { v = v + b.v; return *this; }
    Float& operator-=(Float b) { v = v - b.v; return *this; }
    Float& operator*=(Float b) { v = v * b.v; return *this; }
    Float& operator/=(Float b) { v = v / b.v; return *this; }
};

template <class B> struct Int {
    B v;
    Int() = default;
    template <class T, class = std::enable_if_t<std::is_integral_v<T>>> Int(T i) : v((B)i) {}
    template <class C> Int(Int<C> i) : v((B)i.v) {}
    explicit Int(Float f) : v(std::is_signed_v<B> ? (B)q6_float_to_int(f.v) : (B)q6_float_to_uint(f.v)) {}   /* Q6 */
    explicit Int(double constant) : Int(Float(constant)) {}
    operator B() const { return v; }                        /* subscripts and comparisons use C++'s own integer rules, which are GLSL's */
    Int& operator++() { v = (B)(v + 1); return *this; }
    Int operator++(int) { Int old = *this; v = (B)(v + 1); return old; }
    Int& operator--() { v = (B)(v - 1); return *this; }
    Int operator--(int) { Int old = *this; v = (B)(v - 1); return old; }
    template <class T> Int& operator+=(T b) { *this = *this + b; return *this; }
    template <class T> Int& operator-=(T b) { *this = *this - b; return *this; }
    template <class T> Int& operator*=(T b) { *this = *this * b; return *this; }
    template <class T> Int& operator/=(T b) { *this = *this / b; return *this; }
};
template <class B> Float::Float(Int<B> i) : v((float)i.v) {}

/* int with uint is uint in GLSL and in C++; the arithmetic wraps in 32 bits. */
template <class A, class B> using common_int = std::conditional_t<std::is_signed_v<A> && std::is_signed_v<B>, int32_t, uint32_t>;
template <class R> inline R wrap_add(R a, R b) { return (R)((uint32_t)a + (uint32_t)b); }
template <class R> inline R wrap_sub(R a, R b) { return (R)((uint32_t)a - (uint32_t)b); }
template <class R> inline R wrap_mul(R a, R b) { return (R)((uint32_t)a * (uint32_t)b); }
template <class R> inline R wrap_div(R a, R b) { return (R)(a / b); }
#define GLSL_INT_OP(op, fn)                                                                                                   \
    template <class A, class B> inline Int<common_int<A, B>> operator op(Int<A> a, Int<B> b) {                                \
        using R = common_int<A, B>; return Int<R>(fn<R>((R)a.v, (R)b.v)); }                                                   \
    template <class A, class T, class = std::enable_if_t<std::is_integral_v<T>>>                                              \
    inline Int<common_int<A, T>> operator op(Int<A> a, T b) { using R = common_int<A, T>; return Int<R>(fn<R>((R)a.v, (R)b)); } \
    template <class A, class T, class = std::enable_if_t<std::is_integral_v<T>>>                                              \
    inline Int<common_int<T, A>> operator op(T a, Int<A> b) { using R = common_int<T, A>; return Int<R>(fn<R>((R)a, (R)b.v)); } \
    /* N3: a run-time integer with a floating constant is a binary32 operation */                                             \
    template <class A> inline Float operator op(Int<A> a, double constant) { return Float(a) op Float(constant); }            \
    template <class A> inline Float operator op(double constant, Int<A> b) { return Float(constant) op Float(b); }            \
    template <class A> inline Float operator op(Int<A> a, float b) { return Float(a) op Float(b); }                           \
    template <class A> inline Float operator op(float a, Int<A> b) { return Float(a) op Float(b); }
GLSL_INT_OP(+, wrap_add)
GLSL_INT_OP(-, wrap_sub)
GLSL_INT_OP(*, wrap_mul)
GLSL_INT_OP(/, wrap_div)
#undef GLSL_INT_OP

/* N2: the type of `const float NAME = E;` */
inline double glsl_const(double constant) { return constant; }
inline double glsl_const(int constant) { return (double)constant; }
inline Float glsl_const(Float run_time) { return run_time; }

typedef Int<int32_t> I32;
typedef Int<uint32_t> U32;
inline int32_t to_i32(I32 a) { return a.v; }
inline int32_t to_i32(U32 a) { return (int32_t)a.v; }
template <class T, class = std::enable_if_t<std::is_integral_v<T>>> inline int32_t to_i32(T a) { return (int32_t)a; }

/* ---- vectors --------------------------------------------------------------------------------- */
struct image2D;
struct uvec2 {
    U32 x, y;
    uvec2() = default;
    template <class X, class Y> uvec2(X x_, Y y_) : x((uint32_t)to_i32(x_)), y((uint32_t)to_i32(y_)) {}
};
struct ivec2 {
    I32 x, y;
    ivec2() = default;
    template <class X, class Y> ivec2(X x_, Y y_) : x(to_i32(x_)), y(to_i32(y_)) {}
    explicit ivec2(uvec2 u) : x(to_i32(u.x)), y(to_i32(u.y)) {}
    /* `ivec2 imageSize = imageSize(img);` (img_smooth.comp:21): C++ sees the variable inside its own initialiser,
     * where GLSL still sees the built-in. The call operator makes the line mean what GLSL means. */
    ivec2 operator()(const image2D& img) const;
    friend ivec2 operator+(ivec2 a, ivec2 b) { return ivec2(a.x + b.x, a.y + b.y); }
    friend ivec2 operator*(ivec2 a, int b) { return ivec2(a.x * b, a.y * b); }
};
struct uvec3 {
    U32 x, y, z;
    uvec2 xy;
    uvec3() = default;
    uvec3(uint32_t x_, uint32_t y_, uint32_t z_) : x(x_), y(y_), z(z_), xy(x_, y_) {}
};
struct ivec1 { I32 x; };                                    /* imageSize of a 1-D image is an int; `.x` on a scalar is legal GLSL */
/* The shaders read only `.r` of a loaded texel; the four-component types carry the colour names. */
struct vec4 {
    Float r, g, b, a;
    vec4() = default;
    vec4(Float r_, Float g_, Float b_, Float a_) : r(r_), g(g_), b(b_), a(a_) {}
};
struct uvec4 {
    U32 r, g, b, a;
    uvec4() = default;
    uvec4(U32 r_, U32 g_, U32 b_, U32 a_) : r(r_), g(g_), b(b_), a(a_) {}
    uvec4(Float r_, int g_, int b_, int a_) : r(U32(r_)), g(g_), b(b_), a(a_) {}   /* uvec4(float, 0, 0, 0): Q6 conversion */
};
struct ivec4 {
    I32 r, g, b, a;
    ivec4() = default;
    ivec4(I32 r_, I32 g_, I32 b_, I32 a_) : r(r_), g(g_), b(b_), a(a_) {}
};
struct vec2 {
    Float x, y;
    vec2() = default;
    vec2(Float x_, Float y_) : x(x_), y(y_) {}
};

/* ---- images: views over caller memory --------------------------------------------------------- */
struct image2D {                                            /* r32f (one float per texel) or rgba8 (four bytes per texel) */
    float* f32 = nullptr;
    uint8_t* rgba8 = nullptr;
    int32_t w = 0, h = 0;
};
struct uimage2D {                                           /* r16ui */
    const uint16_t* u16 = nullptr;
    int32_t w = 0, h = 0;
};
struct uimage1D {                                           /* r32ui */
    uint32_t* u32 = nullptr;
    int32_t n = 0;
};
inline ivec2 ivec2::operator()(const image2D& img) const { return ivec2(img.w, img.h); }
inline ivec2 imageSize(const image2D& img) { return ivec2(img.w, img.h); }
inline ivec1 imageSize(const uimage1D& img) { return ivec1{I32(img.n)}; }

inline vec4 imageLoad(const image2D& img, ivec2 p) {
    if (!q1_in_bounds(p.x, p.y, img.w, img.h)) return vec4(0, 0, 0, 0);                       /* Q1 */
    return vec4(img.f32[(size_t)p.y * img.w + p.x], 0, 0, 1);
}
inline uvec4 imageLoad(const uimage2D& img, ivec2 p) {
    if (!q1_in_bounds(p.x, p.y, img.w, img.h)) return uvec4(U32(0u), U32(0u), U32(0u), U32(0u));                  /* Q1 */
    return uvec4(U32((uint32_t)img.u16[(size_t)p.y * img.w + p.x]), U32(0u), U32(0u), U32(1u));
}
inline uvec4 imageLoad(const uimage1D& img, I32 p) {
    if (!q1_in_bounds(p, 0, img.n, 1)) return uvec4(U32(0u), U32(0u), U32(0u), U32(0u));                          /* Q1 */
    return uvec4(U32(img.u32[p.v]), U32(0u), U32(0u), U32(1u));
}
inline uint8_t unorm8(Float c) {
    float v = c.v != c.v ? 0.0f : (c.v < 0.0f ? 0.0f : (c.v > 1.0f ? 1.0f : c.v));
    return (uint8_t)(v * 255.0f + 0.5f);
}
inline void imageStore(const image2D& img, ivec2 p, vec4 value) {
    if (!q1_in_bounds(p.x, p.y, img.w, img.h)) return;                                        /* Q1 */
    size_t i = (size_t)p.y * img.w + p.x;
    if (img.rgba8) {
        img.rgba8[4 * i + 0] = unorm8(value.r); img.rgba8[4 * i + 1] = unorm8(value.g);
        img.rgba8[4 * i + 2] = unorm8(value.b); img.rgba8[4 * i + 3] = unorm8(value.a);
    } else {
        img.f32[i] = value.r.v;
    }
}
inline void imageStore(const image2D& img, ivec2 p, uvec4 value) {
    if (!q1_in_bounds(p.x, p.y, img.w, img.h)) return;                                        /* Q1 */
    img.f32[(size_t)p.y * img.w + p.x] = q4_uvec4_to_r32f(value.r.v);                         /* Q4 */
}
inline U32 imageAtomicAdd(const uimage1D& img, I32 p, U32 add) {
    if (!q1_in_bounds(p, 0, img.n, 1)) return U32(0u);                                        /* Q1 */
    uint32_t old = img.u32[p.v];
    img.u32[p.v] = old + add.v;
    return U32(old);
}

/* ---- built-in functions, as far as the shaders use them ------------------------------------------ */
inline Float sqrt(Float x) { return Float(std::sqrt(x.v)); }                                  /* correctly rounded, as the oracle takes it */
template <class B> inline Float sqrt(Int<B> x) { return sqrt(Float(x)); }
inline Float ceil(Float x) { return Float(std::ceil(x.v)); }
inline Float floor(Float x) { return Float(std::floor(x.v)); }
inline Float abs(Float x) { return Float(std::fabs(x.v)); }
inline Float min(Float x, Float y) { return y < x ? y : x; }                                  /* GLSL 8.3 */
inline Float max(Float x, Float y) { return x < y ? y : x; }
inline Float clamp(Float x, Float lo, Float hi) { return min(max(x, lo), hi); }               /* Q3 */
inline I32 clamp(I32 x, I32 lo, I32 hi) { return x < lo ? lo : (x > hi ? hi : x); }
inline Float pow(Float x, Float y) { return Float(q5_pow(x.v, y.v)); }                        /* Q5 */

/* ---- invocation state: one thread at a time, set by ref_shaders.cpp's dispatcher ------------------ */
inline uvec3 gl_GlobalInvocationID, gl_LocalInvocationID, gl_WorkGroupID, gl_NumWorkGroups;

}  // namespace glsl
#endif
