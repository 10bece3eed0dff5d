// The argument vocabulary of csrc/bindings.cpp: the only place a tensor becomes a pointer.
//
// A ds2_* launcher takes raw pointers and launches on the current device's stream, so every
// tensor argument must be on that device, of the dtype, element count and layout the kernel
// assumes. A binding states that once per argument,
//
//   const Op op{"bn_apply"};
//   const float* mean = op.f32(mean_t, "mean", "C", exactly(C));
//
// and the helper checks it all and returns the typed pointer, or refuses with
//   <op>: <argument> must be <dtype> [<shape>] ..., got ...
// The message is put together only on failure (TORCH_CHECK takes the pieces). Host only.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>

using OptT = c10::optional<at::Tensor>;

// how many elements an argument must have: exactly n, or n or more (workspaces, partials,
// state a longer launch saved: the binding's comment says which)
struct Count {
  int64_t n;
  bool or_more;
};
inline Count exactly(int64_t n) { return {n, false}; }
inline Count at_least(int64_t n) { return {n, true}; }

inline Count whole(const at::Tensor& t) { return {t.numel(), false}; }  // its own sizes define the problem

constexpr at::ScalarType kAnyDtype = at::ScalarType::Undefined;

inline bool has(const OptT& t) { return t.has_value() && t->defined(); }

struct Act {  // an fp32-or-bf16 activation
  void* p;
  int bf16;
};
struct Pitched {  // rows of unit-stride elements, ld elements apart; batches bs elements apart
  void* p;
  int64_t ld, bs;
};

struct Op {
  const char* op;
  // PyTorch's current stream, which the launch goes to, and with it the current device: looked
  // up once per call (the runtime query costs more than every other check of an argument together)
  mutable c10::optional<c10::hip::HIPStream> cur = c10::nullopt;

  const c10::hip::HIPStream& current() const {
    if (!cur.has_value()) cur = c10::hip::getCurrentHIPStream();
    return *cur;
  }
  hipStream_t stream() const { return current().stream(); }

  // on a GPU, and on the one the launch goes to
  void on_device(const at::Tensor& t, const char* name) const {
    TORCH_CHECK(t.is_cuda() && t.get_device() == current().device_index(), op, ": ", name,
                " must be on the current GPU, got a tensor on ", t.device());
  }

  // before any size(i): an argument whose own sizes define the problem has nd dimensions
  void dims(const at::Tensor& t, const char* name, int64_t nd, const char* shape) const {
    TORCH_CHECK(t.dim() == nd, op, ": ", name, " must be [", shape, "], got ", t.sizes());
  }

  // Contiguous device array: dtype (kAnyDtype: whatever it is), element count, byte alignment.
  void* raw(const at::Tensor& t, const char* name, at::ScalarType dtype, const char* shape, Count c,
            int align = 0) const {
    on_device(t, name);
    const int64_t n = t.numel();
    TORCH_CHECK((dtype == kAnyDtype || t.scalar_type() == dtype) && t.is_contiguous() && (c.or_more ? n >= c.n : n == c.n) &&
                    (align == 0 || reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0),
                op, ": ", name, " must be ", dtype == kAnyDtype ? t.scalar_type() : dtype, " [", shape,
                c.or_more ? " or more]" : "]", " = ", c.n, " contiguous elements", align ? ", aligned to " : "",
                align ? std::to_string(align) : std::string(), align ? " bytes" : "", ", got ", t.scalar_type(), " ", t.sizes(),
                t.is_contiguous() ? "" : " (not contiguous)");
    return t.data_ptr();
  }
  void* raw(const OptT& t, const char* name, at::ScalarType dtype, const char* shape, Count c, int align = 0) const {
    return has(t) ? raw(*t, name, dtype, shape, c, align) : nullptr;
  }

  // the dtypes the kernels take; each also for an optional argument (None: nullptr)
  template <typename A> float* f32(const A& t, const char* name, const char* shape, Count c, int align = 0) const {
    return static_cast<float*>(raw(t, name, at::kFloat, shape, c, align));
  }
  template <typename A> int* i32(const A& t, const char* name, const char* shape, Count c, int align = 0) const {
    return static_cast<int*>(raw(t, name, at::kInt, shape, c, align));
  }
  template <typename A> unsigned* u32(const A& t, const char* name, const char* shape, Count c) const {  // int32 words
    return static_cast<unsigned*>(raw(t, name, at::kInt, shape, c));
  }
  template <typename A> void* bf16(const A& t, const char* name, const char* shape, Count c, int align = 0) const {
    return raw(t, name, at::kBFloat16, shape, c, align);
  }
  template <typename A> void* u8(const A& t, const char* name, const char* shape, Count c, int align = 0) const {
    return raw(t, name, at::kByte, shape, c, align);
  }
  template <typename A> long long* i64(const A& t, const char* name, const char* shape, Count c) const {
    return static_cast<long long*>(raw(t, name, at::kLong, shape, c));
  }

  Act act(const at::Tensor& t, const char* name, const char* shape, Count c, int align = 0) const {
    TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16, op, ": ", name,
                " must be float32 or bfloat16 [", shape, "], got ", t.scalar_type());
    return {raw(t, name, t.scalar_type(), shape, c, align), t.scalar_type() == at::kBFloat16 ? 1 : 0};
  }

  // 2-D or batched 3-D operand whose last dimension is unit-stride (rows may be pitched); the
  // caller compares sizes(). ld_mult: the row stride must be a multiple of that many elements.
  Pitched pitched(const at::Tensor& t, const char* name, at::ScalarType dtype, int align = 0, int ld_mult = 1,
                  bool batched = true) const {
    on_device(t, name);
    const int64_t d = t.dim();
    TORCH_CHECK((dtype == kAnyDtype || t.scalar_type() == dtype) && (d == 2 || (batched && d == 3)) && t.stride(-1) == 1 &&
                    (align == 0 || reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0) && t.stride(-2) % ld_mult == 0,
                op, ": ", name, " must be ", dtype == kAnyDtype ? t.scalar_type() : dtype, batched ? " 2-D or batched 3-D" : " 2-D",
                " with a unit-stride last dimension, aligned to ", align, " bytes, row stride a multiple of ", ld_mult,
                " elements, got ", t.scalar_type(), " ", t.sizes(), " strides ", t.strides());
    return {t.data_ptr(), t.stride(-2), d == 3 && t.size(0) > 1 ? t.stride(0) : 0};
  }

  // one fp32 scalar on the device (None: nullptr)
  const float* scalar(const OptT& t, const char* name, Count c = at_least(1)) const { return f32(t, name, "1", c); }
  // the optional per-row lengths int32 [B] (None: every row whole)
  const int* lens(const OptT& t, const char* name, int64_t B) const { return i32(t, name, "B", exactly(B)); }
  // seeds, steps and offsets cross the boundary as 32-bit words
  unsigned word(int64_t v, const char* name) const {
    TORCH_CHECK(v >= 0 && v <= 0xffffffffLL, op, ": ", name, " must be a 32-bit word, got ", v);
    return (unsigned)v;
  }

  void launched(int rc) const { TORCH_CHECK(rc == 0, "deepspeech_amd kernel launch failed in ", op, " (code ", rc, ")"); }
};
