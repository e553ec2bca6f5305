// device_call.h -- how a method of flan::Audio, flan::PV or flan::SPV calls the device: one type for a Function argument as the C ABI takes
// it, and one skeleton for everything after "the method has decided to run".  Private to the host library.
#pragma once
#include <vector>

#include "device_block.h"

namespace flan { namespace detail {

// host memory into a fresh device block through the null stream; the staging block behind `host` may go back to its cache after this
inline std::shared_ptr<DeviceBlock> upload( const void * host, size_t bytes )
	{
	auto b = DeviceBlock::allocate( bytes );
	if( !b ) return nullptr;
	if( !report( flanhip_memcpy_h2d( b->ptr, host, bytes, nullptr ), "upload" ) ) return nullptr;
	if( !report( flanhip_stream_synchronize( nullptr ), "upload" ) ) return nullptr;
	return b;
	}

// A Function as the device entry points take it: a row or grid on the device, or null and a scalar.  A constant allocates nothing.
struct DeviceArg
	{
	std::shared_ptr<DeviceBlock> block;
	float scalar = 0.0f;
	bool ok = true;
	DeviceArg() = default;
	explicit DeviceArg( float constant ) : scalar( constant ) {}
	explicit DeviceArg( std::shared_ptr<DeviceBlock> uploaded ) : block( std::move( uploaded ) ), ok( bool( block ) ) {}   // from upload() or a grid sampler
	// host values through flanhip_upload (synchronous); `what` names them in the one line a failure prints
	static DeviceArg from_host( const void * values, size_t bytes, const char * what )
		{
		DeviceArg a( DeviceBlock::allocate( bytes ) );
		if( a.ok && !( a.ok = upload_from_host( a.block->ptr, values, bytes ) ) )
			std::cerr << "flan: upload of " << what << " failed: " << flanhip_last_error() << std::endl;
		return a;
		}
	template<typename T = float> const T * ptr() const { return block ? static_cast<const T*>( block->ptr ) : nullptr; }
	};

// One call of the device.  The method names what the launch needs (need() for an input's device_data() and an argument's ok, output(),
// workspace(), scratch()), passes ok(), hands every launch's return code to launch() and returns finish().
// The rule it keeps, on which the cache of idle blocks rests (host_runtime.cpp): from the first successful launch on, every way out of the
// method -- finish(), a `return` after a later failure, an exception -- synchronises the null stream BEFORE a block goes back to the cache.
// The destructor's body does that, so the blocks held here go after it; declare the DeviceCall AFTER the arguments and temporaries its
// launches read, so that it is destroyed before them.  Before the first launch nothing is synchronised.
class DeviceCall
	{
public:
	explicit DeviceCall( const char * who ) : who_( who ) {}
	DeviceCall( const DeviceCall & ) = delete;
	DeviceCall & operator=( const DeviceCall & ) = delete;
	~DeviceCall() { if( in_flight_ ) (void) flanhip_stream_synchronize( nullptr ); }

	bool ok() const { return ok_; }
	bool need( bool have ) { ok_ = ok_ && have; return have; }
	// the block finish() hands over, as `count` T
	template<typename T> T * output( size_t count ) { return static_cast<T*>( held( out_ = DeviceBlock::allocate( sizeof( T ) * count ) ) ); }
	// a further block that lives as long as the call
	void * scratch( size_t bytes ) { scratch_.push_back( DeviceBlock::allocate( bytes ) ); return held( scratch_.back() ); }
	// 0 bytes refuses the call, silently: the C ABI's answer to a shape it does not take.  `optional`: 0 bytes, or no memory, is no failure --
	// the method runs unfused, with a null workspace
	void * workspace( size_t bytes, bool optional = false )
		{
		if( bytes ) ws_ = DeviceBlock::allocate( bytes );
		return optional ? ( ws_ ? ws_->ptr : nullptr ) : held( ws_ );
		}
	// what a launch returned, reported under the method's name; from the first FLANHIP_OK on the device counts as busy
	bool launch( int rc ) { in_flight_ = in_flight_ || rc == FLANHIP_OK; return need( report( rc, who_ ) ); }
	// The cancellable conversions wait here, not in finish(): the flag is polled during the wait and stops the kernels that read it.  The answer
	// comes back unreported, for the method to say what a raised flag means; sync() and finish() report it and wait for nothing twice
	int wait( std::atomic<bool> & canceller )
		{
		waited_ = flanhip_wait_cancellable_fn( nullptr, poll_canceller, &canceller );
		in_flight_ = waited_ != FLANHIP_OK && waited_ != FLANHIP_ERR_CANCELLED;       // after either of the two the stream has drained
		has_waited_ = true;
		return waited_;
		}
	// the one synchronise of the success path, reported
	bool sync()
		{
		if( !has_waited_ ) { waited_ = flanhip_stream_synchronize( nullptr ); in_flight_ = false; has_waited_ = true; }
		return need( report( waited_, who_ ) );
		}
	// the output block as a Buffer of format f, not waited for: split_channels hands out one per channel, then sync()s once
	template<typename Buffer> Buffer adopt( const typename Buffer::Format & f ) { return Buffer::adopt_device( f, std::move( out_ ) ); }
	// a null Buffer if anything was missing or failed; else one synchronise, and the output block is handed over
	template<typename Buffer> Buffer finish( const typename Buffer::Format & f ) { return ok_ && sync() ? adopt<Buffer>( f ) : Buffer(); }
	// finish(), and the workspace the launch filled goes with the result (PVBuffer::attach_synthesis_workspace)
	template<typename Buffer> Buffer finish_fused( const typename Buffer::Format & f, bool maybe = false )
		{
		Buffer out = finish<Buffer>( f );
		if( ok_ && ws_ ) out.attach_synthesis_workspace( std::move( ws_ ), maybe );
		return out;
		}

private:
	void * held( const std::shared_ptr<DeviceBlock> & b ) { return need( bool( b ) ) ? b->ptr : nullptr; }
	const char * who_;
	bool ok_ = true, in_flight_ = false, has_waited_ = false;
	int waited_ = FLANHIP_OK;
	std::shared_ptr<DeviceBlock> out_, ws_;
	std::vector<std::shared_ptr<DeviceBlock>> scratch_;
	};

constexpr size_t kNoWorkspace = ~size_t( 0 );

// The common case in one expression: with every requirement in `have`, one launch( out, ws ) into a fresh block of `count` T beside a
// workspace of ws_bytes (0 refuses; kNoWorkspace: none), one synchronise, the block adopted with format f.
template<typename Buffer, typename T, typename Launch>
Buffer device_call( const char * who, const typename Buffer::Format & f, size_t count, bool have, size_t ws_bytes, Launch launch )
	{
	DeviceCall call( who );
	call.need( have );
	T * out = call.template output<T>( count );
	void * ws = ws_bytes == kNoWorkspace ? nullptr : call.workspace( ws_bytes );
	if( call.ok() ) call.launch( launch( out, ws ) );
	return call.template finish<Buffer>( f );
	}

} }
