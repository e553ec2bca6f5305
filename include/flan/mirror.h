// flan/mirror.h -- the lazily mirrored storage under AudioBuffer, PVBuffer and SPVBuffer: a host vector and a block of HBM, either of
// which may hold the only current copy.  Results of device algorithms stay in HBM until host code asks for the elements; host data goes
// up when a device algorithm first needs it.  The owner passes the element count in (it follows from the owner's Format).
#pragma once
#include <cstddef>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace flan { namespace detail {

struct DeviceBlock;                                // flan_amd/host/device_block.h

// The lock that guards an object's lazily mirrored state (host copy <-> HBM copy, attached workspaces).
// The reference's const methods are pure reads and may run concurrently on one object; here a const method may bring the host copy
// over from the device, upload it, or hand a workspace on, so those steps take this per-object mutex.  The buffers are move-only
// with defaulted moves: a moved-to object simply gets a fresh, unlocked mutex (nobody may be using either object during a move).
struct MirrorLock
	{
	mutable std::mutex m;
	MirrorLock() = default;
	MirrorLock( const MirrorLock & ) {}
	MirrorLock( MirrorLock && ) noexcept {}
	MirrorLock & operator=( const MirrorLock & ) { return *this; }
	MirrorLock & operator=( MirrorLock && ) noexcept { return *this; }
	std::unique_lock<std::mutex> hold() const { return std::unique_lock<std::mutex>( m ); }
	};

template<typename T>                               // float and MF (flan_amd/host/Mirror.cpp)
class Mirror
	{
public:
	/** noun: what the transfer-failure messages call the data.  lazy_zeros: a current host copy that does not hold `count` elements
	 *  stands for zeros that take no memory until they are touched; without it such a copy is simply what it is (empty after a move). */
	explicit Mirror( const char * noun, bool lazy_zeros = false, std::vector<T> host = {} )
		: noun( noun ), lazy_zeros( lazy_zeros ), buffer( std::move( host ) ) {}

	Mirror copy( size_t count ) const { return Mirror( noun, lazy_zeros, host( count ) ); }   // deep copy, host side only
	void adopt( std::shared_ptr<DeviceBlock> block ) { dev = std::move( block ); host_valid = false; }   // the HBM copy is the truth

	// Every method below takes the lock once.  The writing ones also drop *derived under that hold: device state the owner
	// computed from the old data and guards with hold() (PVBuffer's synthesis workspace).
	void clear( size_t count, std::shared_ptr<DeviceBlock> * derived = nullptr );
	const std::vector<T> & host( size_t count ) const;      // downloads from HBM on first use: the first caller does, the others wait
	std::vector<T> & host( size_t count, std::shared_ptr<DeviceBlock> * derived = nullptr );   // ... and drops the device copy: the caller may write
	std::shared_ptr<DeviceBlock> device_block( size_t count ) const;   // uploads on first use; nullptr on failure, or if the host copy is short
	const T * device_data( size_t count ) const;
	bool is_device_resident() const { auto held = hold(); return bool( dev ); }
	bool host_copy_is_current() const { auto held = hold(); return host_valid; }            // false: the data lives on the device only
	bool holds_nothing() const { auto held = hold(); return host_valid && buffer.empty() && !dev; }
	std::unique_lock<std::mutex> hold() const { return lock.hold(); }

private:
	void materialize( size_t count ) const;        // the host copy, whole (lock held)
	const char * noun;
	bool lazy_zeros;
	mutable std::vector<T> buffer;
	mutable bool host_valid = true;
	mutable std::shared_ptr<DeviceBlock> dev;
	MirrorLock lock;
	};

} }
