// device_call_test -- the rule flan_amd/host/device_call.h keeps, checked on a log of events without a device and without either library:
// from the first successful launch on, every way out of a method synchronises the null stream before a block goes back to the cache;
// before the first launch nothing is synchronised; the success path synchronises exactly once and hands the output block over.
// The few symbols the header references are defined here as stand-ins that append to the log.
#include <algorithm>
#include <cstdio>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_call.h"

using namespace flan::detail;

static std::vector<std::string> events;
static int acquired = 0, refuse_acquire = 0, sync_answer = FLANHIP_OK, wait_answer = FLANHIP_OK, failures = 0;

static void note( const std::string & what, const void * block = nullptr ) { events.push_back( block ? what + ":" + std::to_string( reinterpret_cast<size_t>( block ) ) : what ); }

namespace flan { namespace detail {
void * device_acquire( size_t, size_t * capacity, int * device )       // block k is the pointer k; refuse_acquire = k: the k-th request gets nothing
	{
	if( ++acquired == refuse_acquire ) { note( "refused" ); return nullptr; }
	*capacity = 4096; *device = 0;
	void * p = reinterpret_cast<void*>( size_t( acquired ) );
	note( "acquire", p );
	return p;
	}
void device_release( void * ptr, size_t, int ) noexcept { note( "release", ptr ); }
} }
extern "C" {
const char * flanhip_last_error( void ) { return "stand-in"; }
int flanhip_stream_synchronize( void * ) { note( "sync" ); return sync_answer; }
int flanhip_wait_cancellable_fn( void *, int ( * )( void * ), void * ) { note( "wait" ); return wait_answer; }
}

struct Buffer                                                              // what the skeleton needs of AudioBuffer / PVBuffer / SPVBuffer
	{
	struct Format { int frames = 0; };
	Format format;
	std::shared_ptr<DeviceBlock> block;
	static Buffer adopt_device( const Format & f, std::shared_ptr<DeviceBlock> b ) { note( "adopt", b->ptr ); Buffer out; out.format = f; out.block = std::move( b ); return out; }
	};

static long count( const std::string & e ) { return std::count( events.begin(), events.end(), e ); }
static long at( const std::string & e ) { return std::find( events.begin(), events.end(), e ) - events.begin(); }       // events.size() when absent
static long first_release() { return std::find_if( events.begin(), events.end(), []( const std::string & e ){ return e.rfind( "release", 0 ) == 0; } ) - events.begin(); }
static std::string joined() { std::string s; for( const auto & e : events ) s += e + " "; return s; }

#define CHECK( cond ) do { if( !( cond ) ) { ++failures; std::printf( "FAILED %s:%d: %s\n    log: %s\n", __FILE__, __LINE__, #cond, joined().c_str() ); } } while( 0 )

static void reset( int refuse = 0 ) { events.clear(); acquired = 0; refuse_acquire = refuse; sync_answer = wait_answer = FLANHIP_OK; }
static int launch_ok() { note( "launch" ); return FLANHIP_OK; }

// every block acquired went back, once
static void check_all_released()
	{
	for( const auto & e : events ) if( e.rfind( "acquire:", 0 ) == 0 ) CHECK( count( "release:" + e.substr( 8 ) ) == 1 );
	}

// ... and, after a launch, not before the one synchronise
static void check_all_released_after_one_sync()
	{
	CHECK( count( "sync" ) == 1 && at( "launch" ) < at( "sync" ) && at( "sync" ) < first_release() );
	check_all_released();
	}

int main()
	{
	const Buffer::Format f{ 7 };
	std::stringstream reported;
	std::streambuf * const stderr_buf = std::cerr.rdbuf( reported.rdbuf() );       // what report() and DeviceBlock::allocate print

	// (a) success: one synchronise, before the workspace and the argument go back; the output block is not released but handed over
	reset();
		{
		Buffer out;
			{
			const DeviceArg arg( DeviceBlock::allocate( 64 ) );                     // block 1
			out = device_call<Buffer, float>( "a", f, 16, arg.ok, 128, [&]( float * o, void * ws )   // output: block 2, workspace: block 3
				{ CHECK( o == reinterpret_cast<float*>( size_t( 2 ) ) && ws == reinterpret_cast<void*>( size_t( 3 ) ) ); return launch_ok(); } );
			}
		CHECK( count( "sync" ) == 1 && count( "launch" ) == 1 );
		CHECK( at( "launch" ) < at( "sync" ) && at( "sync" ) < at( "release:3" ) && at( "sync" ) < at( "release:1" ) );
		CHECK( count( "release:1" ) == 1 && count( "release:3" ) == 1 && count( "release:2" ) == 0 );
		CHECK( count( "adopt:2" ) == 1 && at( "sync" ) < at( "adopt:2" ) );
		CHECK( out.block && out.block->ptr == reinterpret_cast<void*>( size_t( 2 ) ) && out.format.frames == 7 );
		}
	CHECK( count( "release:2" ) == 1 );                                           // (the result's own end)
	CHECK( reported.str().empty() );

	// (b) a failure before any launch: nothing is launched or synchronised, every block acquired so far goes back, the result is null
	const DeviceArg failed_upload( std::shared_ptr<DeviceBlock>{} );
	CHECK( !failed_upload.ok && DeviceArg( 2.5f ).ok && DeviceArg( 2.5f ).scalar == 2.5f && !DeviceArg( 2.5f ).ptr() );
	struct { const char * name; bool have; int refuse; size_t ws_bytes; } before[] = {
		{ "a missing input", false, 0, 128 }, { "an argument that is not ok", failed_upload.ok, 0, 128 },
		{ "a refused output", true, 1, 128 }, { "a refused workspace", true, 2, 128 }, { "a workspace of 0 bytes", true, 0, 0 } };
	for( const auto & b : before )
		{
		reset( b.refuse );
		const Buffer out = device_call<Buffer, float>( b.name, f, 16, b.have, b.ws_bytes, [&]( float *, void * ){ return launch_ok(); } );
		CHECK( !out.block && count( "sync" ) == 0 && count( "launch" ) == 0 && count( "adopt:1" ) == 0 && first_release() < long( events.size() ) );
		check_all_released();
		}
	// (an optional workspace is no requirement: 0 bytes and a refused allocation both run, unfused)
	for( int refuse = 0; refuse <= 2; refuse += 2 )
		{
		reset( refuse );
		DeviceCall call( "optional" );
		call.output<float>( 16 );
		CHECK( call.workspace( refuse ? 128 : 0, true ) == nullptr && call.ok() );
		}

	// (c) a failure after a launch -- a second launch's error code, or a refused allocation: one synchronise before the first release
	reset();
		{
		DeviceCall call( "c1" );
		call.scratch( 64 ); call.output<float>( 16 ); call.workspace( 128 );
		CHECK( call.launch( launch_ok() ) && !call.launch( FLANHIP_ERR_HIP ) && !call.ok() );
		CHECK( !call.finish<Buffer>( f ).block );
		CHECK( count( "sync" ) == 0 );                                             // (not yet: the way out does it)
		}
	check_all_released_after_one_sync();
	reset( 2 );
		{
		DeviceCall call( "c2" );
		call.scratch( 64 );
		CHECK( call.launch( launch_ok() ) );
		CHECK( call.output<float>( 16 ) == nullptr && !call.ok() );
		}
	check_all_released_after_one_sync();

	// (d) an exception between a launch and the finish: as (c)
	reset();
	try
		{
		DeviceCall call( "d" );
		call.scratch( 64 ); call.output<float>( 16 );
		call.launch( launch_ok() );
		throw std::runtime_error( "the user's callable" );
		}
	catch( const std::runtime_error & ) { note( "caught" ); }
	check_all_released_after_one_sync();
	CHECK( first_release() < at( "caught" ) );

	// (e) a failing synchronise on the success path: a null result, one reported line, no second synchronise
	reset();
	reported.str( "" );
	sync_answer = FLANHIP_ERR_HIP;
		{
		const Buffer out = device_call<Buffer, float>( "e", f, 16, true, kNoWorkspace, [&]( float *, void * ws ){ CHECK( !ws ); return launch_ok(); } );
		CHECK( !out.block && count( "adopt:1" ) == 0 );
		}
	check_all_released_after_one_sync();
	const std::string line = reported.str();
	CHECK( std::count( line.begin(), line.end(), '\n' ) == 1 && line.find( "flan: e failed (-3)" ) == 0 );

	// the cancellable wait takes the synchronise's place: OK -- finish() waits for nothing more; cancelled -- the stream has drained, the way
	// out waits for nothing; failed -- the way out synchronises
	for( int answer : { FLANHIP_OK, FLANHIP_ERR_CANCELLED, FLANHIP_ERR_HIP } )
		{
		reset();
		wait_answer = answer;
		std::atomic<bool> canceller( false );
			{
			DeviceCall call( "wait" );
			call.output<float>( 16 );
			call.launch( launch_ok() );
			CHECK( call.wait( canceller ) == answer );
			CHECK( bool( call.finish<Buffer>( f ).block ) == ( answer == FLANHIP_OK ) );
			}
		CHECK( count( "wait" ) == 1 && count( "sync" ) == ( answer == FLANHIP_ERR_HIP ? 1 : 0 ) && count( "release:1" ) == 1 );
		if( answer == FLANHIP_ERR_HIP ) CHECK( at( "sync" ) < first_release() );
		}

	std::cerr.rdbuf( stderr_buf );
	std::printf( failures ? "%d check(s) FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
