/* hc-mvs_amd/csrc/dev_buf.h -- the owners of what the library takes from the runtime: a grow-only device buffer with the out-of-memory
 * hook and the carving of one allocation into pieces (carve.h), a grow-only page-locked host buffer, an event */
#ifndef HCMVS_DEV_BUF_H
#define HCMVS_DEV_BUF_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "carve.h"
namespace hcmvs {

// Gives device memory back when an allocation fails; returns whether it freed anything (the allocation is then tried once more)
struct Reclaimer {
	virtual bool reclaim() = 0;
protected:
	~Reclaimer() = default;
};

// A device allocation, freed when the buffer goes.  reserve() only grows: a larger request waits for the stream (work in flight
// may still use the old allocation), frees it and allocates exactly the bytes asked for -- the contents are not kept.
class DevBuf {
public:
	DevBuf() = default;
	explicit DevBuf(Reclaimer* r) : rec_(r) {}
	DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_), rec_(o.rec_) { o.p_ = nullptr; o.cap_ = 0; }
	DevBuf& operator=(DevBuf&& o) noexcept {
		if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; rec_ = o.rec_; o.p_ = nullptr; o.cap_ = 0; }
		return *this;
	}
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { reset(); }

	hipError_t reserve(size_t bytes, hipStream_t s) {
		if (bytes <= cap_) return hipSuccess;
		if (p_) {
			const hipError_t e = hipStreamSynchronize(s);
			if (e != hipSuccess) return e;
		}
		reset();
		hipError_t e = hipMalloc(&p_, bytes);
		if (e != hipSuccess && rec_) { (void)hipGetLastError(); if (rec_->reclaim()) e = hipMalloc(&p_, bytes); }
		if (e != hipSuccess) { (void)hipGetLastError(); p_ = nullptr; return e; }
		cap_ = bytes;
		return hipSuccess;
	}
	void reset() {
		if (p_) (void)hipFree(p_);
		p_ = nullptr; cap_ = 0;
	}
	template <class T = char> T* get() const { return (T*)p_; }
	size_t capacity() const { return cap_; }

private:
	void* p_ = nullptr;
	size_t cap_ = 0;
	Reclaimer* rec_ = nullptr;
};

// A page-locked host allocation, freed when the buffer goes.  reserve() only grows, to exactly the bytes asked for; the contents are
// not kept, and whoever grows it knows that no copy out of it is in flight.
class PinnedBuf {
public:
	PinnedBuf() = default;
	PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	PinnedBuf& operator=(PinnedBuf&& o) noexcept {
		if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
		return *this;
	}
	PinnedBuf(const PinnedBuf&) = delete;
	PinnedBuf& operator=(const PinnedBuf&) = delete;
	~PinnedBuf() { reset(); }

	hipError_t reserve(size_t bytes) {
		if (bytes <= cap_) return hipSuccess;
		reset();
		const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
		if (e != hipSuccess) { (void)hipGetLastError(); p_ = nullptr; return e; }
		cap_ = bytes;
		return hipSuccess;
	}
	void reset() {
		if (p_) (void)hipHostFree(p_);
		p_ = nullptr; cap_ = 0;
	}
	char* get() const { return (char*)p_; }
	size_t capacity() const { return cap_; }

private:
	void* p_ = nullptr;
	size_t cap_ = 0;
};

// An event, created with its flags when it is first asked for and destroyed when the owner goes
class Event {
public:
	explicit Event(unsigned flags = hipEventDefault) : flags_(flags) {}
	Event(Event&& o) noexcept : e_(o.e_), flags_(o.flags_) { o.e_ = nullptr; }
	Event& operator=(Event&& o) noexcept {
		if (this != &o) { reset(); e_ = o.e_; flags_ = o.flags_; o.e_ = nullptr; }
		return *this;
	}
	Event(const Event&) = delete;
	Event& operator=(const Event&) = delete;
	~Event() { reset(); }

	hipError_t ensure() { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags_); }
	void reset() {
		if (e_) (void)hipEventDestroy(e_);
		e_ = nullptr;
	}
	hipEvent_t get() const { return e_; }

private:
	hipEvent_t e_ = nullptr;
	unsigned flags_;
};

} // namespace hcmvs
#endif
