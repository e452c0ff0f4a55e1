// dev_buf.h -- the one owner of a device or pinned-host allocation of the context (ebo_ctx.h): a pointer and a
// capacity in ELEMENTS of T (bytes for void and char), released by the destructor.  Header-only and free of HIP --
// the memory comes from a policy `Mem` with `static void* allocate(size_t bytes)` (nullptr on failure) and
// `static void release(void*)` -- so that the grow rule below, the only copy of it, is tested on the CPU under
// AddressSanitizer with a counting policy (tests/cpp/dev_buf_test.cpp, tests/test_dev_buf_cpu.py).
#pragma once

#include <stddef.h>

#include <utility>

namespace ebo
{
enum class Grow
{
	kOk,       // the buffer holds at least what was asked for
	kRefused,  // it does not, and allocating was not allowed: nothing changed
	kFailed,   // the allocation failed: the buffer is empty
};

template <class T>
inline constexpr size_t kElemBytes = sizeof(T);
template <>
inline constexpr size_t kElemBytes<void> = 1;

template <class T, class Mem>
class DevBuf
{
   public:
	DevBuf() = default;
	DevBuf(DevBuf&& o) noexcept { swap(o); }
	DevBuf& operator=(DevBuf&& o) noexcept
	{
		DevBuf taken(std::move(o));
		swap(taken);
		return *this;
	}
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { reset(); }

	T* get() const { return p_; }
	operator T*() const { return p_; }  // the call sites pass and index the member as the pointer it was
	size_t cap() const { return cap_; }

	// At least n elements; contents are not kept.  A buffer that fits keeps its pointer (a recorded graph holds it).
	// One that does not is released FIRST and then allocated, so the peak is the larger of the two, not their sum.
	Grow ensure(size_t n, bool mayAllocate = true)
	{
		if (n <= cap_)
		{
			return Grow::kOk;
		}
		if (!mayAllocate)
		{
			return Grow::kRefused;
		}
		reset();
		p_ = static_cast<T*>(Mem::allocate(n * kElemBytes<T>));
		if (!p_)
		{
			return Grow::kFailed;
		}
		cap_ = n;
		return Grow::kOk;
	}
	void reset()
	{
		if (p_)
		{
			Mem::release(p_);
		}
		p_ = nullptr;
		cap_ = 0;
	}
	void swap(DevBuf& o) noexcept
	{
		std::swap(p_, o.p_);
		std::swap(cap_, o.cap_);
	}

   private:
	T* p_ = nullptr;
	size_t cap_ = 0;
};

// Three blocks with one logical size (the pinned staging of an evaluation round): afterwards each holds its count, or
// -- when one allocation fails -- all three are empty.  All are released before the first allocation.
template <class A, class B, class C>
Grow ensure3(A& a, size_t na, B& b, size_t nb, C& c, size_t nc, bool mayAllocate = true)
{
	if (na <= a.cap() && nb <= b.cap() && nc <= c.cap())
	{
		return Grow::kOk;
	}
	if (!mayAllocate)
	{
		return Grow::kRefused;
	}
	a.reset();
	b.reset();
	c.reset();
	if (a.ensure(na) == Grow::kOk && b.ensure(nb) == Grow::kOk && c.ensure(nc) == Grow::kOk)
	{
		return Grow::kOk;
	}
	a.reset();
	b.reset();
	c.reset();
	return Grow::kFailed;
}
}  // namespace ebo
