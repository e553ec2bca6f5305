// spv_test.cpp -- the C++ sliding-DFT surface (include/flan/SPV.h, SPVBuffer.h, Audio::convert_to_SPV) over libflan_host.so.
//   spv_test --host      format arithmetic and buffer positions (no device needed)
//   spv_test --no-device the conversions return null objects (no CPU fallback)
//   spv_test --device    the classes against the C ABI, bit for bit
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "flan/flan.h"
#include "flanhip.h"

using namespace flan;

static int failures = 0;
#define CHECK( cond ) do { if( !( cond ) ) { std::printf( "FAILED: %s (line %d)\n", #cond, __LINE__ ); ++failures; } } while( 0 )

static bool same_bits( const void * a, const void * b, size_t bytes ) { return std::memcmp( a, b, bytes ) == 0; }

static std::vector<float> noise( size_t n, uint32_t seed )
	{
	std::vector<float> v( n );
	for( size_t i = 0; i < n; ++i ) { seed = seed * 1664525u + 1013904223u; v[i] = float( int32_t( seed >> 8 ) - ( 1 << 23 ) ) / float( 1 << 24 ); }
	return v;
	}

static void host_checks()
	{
	static_assert( !std::is_copy_constructible<SPVBuffer>::value && std::is_move_constructible<SPVBuffer>::value, "move-only" );
	static_assert( !std::is_copy_constructible<SPV>::value, "move-only" );
	SPVBuffer::Format f;
	f.num_channels = 3; f.num_frames = 1000000; f.num_bins = 1024; f.sample_rate = 48000.0f;
	const SPVBuffer s( f );                                    // no memory until touched
	CHECK( !s.is_null() );
	CHECK( SPVBuffer().is_null() );
	CHECK( s.get_analysis_rate() == 48000.0f );
	CHECK( s.bin_to_frequency( 5.0f ) == 5.0f * 48000.0f / 1024.0f );          // b sr / N, not b sr / L
	CHECK( s.bin_to_frequency( 1023.0f ) == 1023.0f * 48000.0f / 1024.0f );
	CHECK( s.frequency_to_bin( 468.75f ) == 468.75f * 1024.0f / 48000.0f );
	CHECK( s.time_to_frame( 0.5f ) == 24000.0f );
	CHECK( s.frame_to_time( 24000.0f ) == 0.5f );
	const size_t pos = s.get_buffer_pos( 2, 999999, 1023 );
	CHECK( pos == ( size_t( 2 ) * 1000000 + 999999 ) * 1024 + 1023 );
	CHECK( pos > ( size_t( 1 ) << 31 ) );
	SPVBuffer::Format g; g.num_channels = 2; g.num_frames = 7; g.num_bins = 3; g.sample_rate = 44100.0f;
	SPV small( g );
	CHECK( small.get_MF( 1, 6, 2 ).m == 0.0f && small.get_MF( 1, 6, 2 ).f == 0.0f );
	small.get_MF( 1, 6, 2 ) = MF{ 1.0f, 2.0f };
	const SPV c = small.copy();
	CHECK( c.get_MF( 1, 6, 2 ).f == 2.0f && c.get_buffer().size() == 42 );
	SPV moved( std::move( small ) );
	CHECK( moved.get_MF( 1, 6, 2 ).m == 1.0f );
	moved.clear_buffer();
	CHECK( moved.get_MF( 1, 6, 2 ).m == 0.0f );
	}

static void no_device_checks()
	{
	Audio a = Audio::create_from_buffer( noise( 2 * 1000, 1 ), 2, 48000.0f );
	CHECK( a.convert_to_SPV( 64 ).is_null() );
	CHECK( a.convert_to_ms_SPV( 64 ).is_null() );
	SPVBuffer::Format g; g.num_channels = 1; g.num_frames = 100; g.num_bins = 8; g.sample_rate = 48000.0f;
	CHECK( SPV( g ).convert_to_audio().is_null() );
	}

static void device_checks()
	{
	const Channel ch = 2;
	const Frame n = 20000;
	const std::vector<float> x = noise( size_t( ch ) * n, 7 );
	Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, 48000.0f );
	CHECK( a.convert_to_SPV( 1 ).is_null() );

	// convert_to_SPV( 1024 ).convert_to_audio() == the C ABI's host forms
	const Bin N = 1024;
	SPV spv = a.convert_to_SPV( N );
	CHECK( !spv.is_null() && spv.is_device_resident() && !spv.host_copy_is_current() );
	std::vector<flanhip_MF> want( size_t( ch ) * n * N );
	CHECK( flanhip_spv_analyze( x.data(), ch, n, 48000.0f, N, want.data(), nullptr ) == FLANHIP_OK );
	Audio out = spv.convert_to_audio();                        // straight from HBM
	CHECK( !out.is_null() && out.get_num_frames() == n && out.get_num_channels() == ch );
	std::vector<float> want_out( size_t( ch ) * n );
	CHECK( flanhip_spv_synthesize( want.data(), ch, n, N, 48000.0f, want_out.data(), nullptr ) == FLANHIP_OK );
	CHECK( same_bits( out.get_buffer().data(), want_out.data(), sizeof( float ) * want_out.size() ) );
	CHECK( same_bits( spv.get_buffer().data(), want.data(), sizeof( MF ) * want.size() ) );

	// convert_to_lr_audio == convert_to_audio().convert_to_left_right()
	const Audio lr = spv.convert_to_lr_audio();
	const Audio lr_want = spv.convert_to_audio().convert_to_left_right();
	CHECK( !lr.is_null() && same_bits( lr.get_buffer().data(), lr_want.get_buffer().data(), sizeof( float ) * lr_want.get_buffer().size() ) );

	// convert_to_ms_SPV == mid / side, then the analysis
	const SPV ms = a.convert_to_ms_SPV( 64 );
	const Audio mid_side = a.convert_to_mid_side();
	std::vector<flanhip_MF> ms_want( size_t( ch ) * n * 64 );
	CHECK( flanhip_spv_analyze( mid_side.get_buffer().data(), ch, n, 48000.0f, 64, ms_want.data(), nullptr ) == FLANHIP_OK );
	CHECK( !ms.is_null() && same_bits( ms.get_buffer().data(), ms_want.data(), sizeof( MF ) * ms_want.size() ) );

	// modify_frequency / repitch: constants on the device, callables on the host, each against its definition
	const SPV small = a.convert_to_SPV( 100 );
	const std::vector<MF> & in = small.get_buffer();
	const SPV fc = small.modify_frequency( 440.5f );
	const SPV rc = small.repitch( 1.25f );
	const SPV fcall = small.modify_frequency( []( TF tf ){ return tf.f * 0.5f + tf.t; } );
	const SPV rcall = small.repitch( []( TF tf ){ return 2.0f + tf.t; } );
	CHECK( !fc.is_null() && !rc.is_null() && !fcall.is_null() && !rcall.is_null() );
	const std::vector<MF> & o1 = fc.get_buffer(), & o2 = rc.get_buffer(), & o3 = fcall.get_buffer(), & o4 = rcall.get_buffer();
	size_t bad = 0;
	for( Channel c = 0; c < ch; ++c )
		for( Frame f = 0; f < n; ++f )
			{
			const Second t = small.frame_to_time( fFrame( f ) );
			for( Bin b = 0; b < 100; ++b )
				{
				const size_t i = small.get_buffer_pos( c, f, b );
				const MF mf = in[i];
				bad += !( o1[i].m == mf.m && o1[i].f == 440.5f );
				bad += !( o2[i].m == mf.m && o2[i].f == mf.f * 1.25f );
				bad += !( o3[i].m == mf.m && o3[i].f == mf.f * 0.5f + t );
				bad += !( o4[i].m == mf.m && o4[i].f == mf.f * ( 2.0f + t ) );
				}
			}
	CHECK( bad == 0 );
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--host";
	host_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		device_checks();
		}
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
