// convolve_test.cpp -- Audio::convolve (include/flan/Audio.h) over libflan_host.so.
//   convolve_test --no-device  null inputs give null Audio, and without a device the call fails loudly with a null result
//   convolve_test --device     against the C ABI bit for bit, the resample rule, the normalize gain, device residency
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static void null_checks()
	{
	const Audio a = Audio::create_from_buffer( noise( 2 * 1000, 1 ), 2, 48000.0f );
	CHECK( a.convolve( Audio() ).is_null() );
	CHECK( Audio().convolve( a ).is_null() );
	}

static void no_device_checks()
	{
	const Audio a = Audio::create_from_buffer( noise( 2 * 1000, 1 ), 2, 48000.0f );
	const Audio h = Audio::create_from_buffer( noise( 100, 2 ), 1, 48000.0f );
	CHECK( a.convolve( h ).is_null() );
	CHECK( a.convolve( h, false ).is_null() );
	}

static void device_checks()
	{
	const Channel ch = 2;
	const Frame n = 50000, m = 7000;
	const std::vector<float> x = noise( size_t( ch ) * n, 7 ), hv = noise( size_t( m ), 8 );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, 48000.0f );
	const Audio h = Audio::create_from_buffer( std::vector<float>( hv ), 1, 48000.0f );

	// Audio::convolve == the C ABI's host form, both normalize settings; the result stays in HBM until read
	for( int normalize = 0; normalize < 2; ++normalize )
		{
		const Audio y = a.convolve( h, normalize != 0 );
		CHECK( !y.is_null() && y.is_device_resident() );
		CHECK( y.get_num_channels() == ch && y.get_num_frames() == n + m && y.get_sample_rate() == 48000.0f );
		std::vector<float> want( size_t( ch ) * ( n + m ) );
		CHECK( flanhip_convolve( x.data(), ch, n, hv.data(), 1, m, 48000.0f, normalize, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_bits( y.get_buffer().data(), want.data(), sizeof( float ) * want.size() ) );
		}

	// normalize: convolve( ir, false ) times 1.0f / get_max_sample_magnitude(), bit for bit
		{
		const Audio raw = a.convolve( h, false );
		const Audio nrm = a.convolve( h, true );
		const float gain = 1.0f / raw.get_max_sample_magnitude();
		const std::vector<float> & r = raw.get_buffer(), & q = nrm.get_buffer();
		size_t bad = 0;
		for( size_t i = 0; i < r.size(); ++i ) { const float v = r[i] * gain; bad += !same_bits( &v, &q[i], sizeof( float ) ); }
		CHECK( bad == 0 );
		}

	// an IR of another rate: resampled to this one first
		{
		const Audio h44 = Audio::create_from_buffer( noise( 2 * 4410, 9 ), 2, 44100.0f );
		const Audio y = a.convolve( h44, false );
		const Audio h48 = h44.resample( 48000.0f );
		const Audio want = a.convolve( h48, false );
		CHECK( !y.is_null() && !want.is_null() && y.get_num_frames() == n + h48.get_num_frames() );
		CHECK( y.get_sample_rate() == 48000.0f && y.get_num_channels() == ch );
		CHECK( same_bits( y.get_buffer().data(), want.get_buffer().data(), sizeof( float ) * want.get_buffer().size() ) );
		}

	// a chain that never leaves the device until the end: convolve, then convert_to_PV
		{
		const Audio y = a.convolve( h );
		CHECK( y.is_device_resident() );
		const PV pv = y.convert_to_PV( 2048, 512, 2048 );
		CHECK( !pv.is_null() && pv.is_device_resident() );
		}

	// silence: zeros without normalize, NaN with it (the reference multiplies by 1.0f / 0)
		{
		const Audio z = Audio::create_from_buffer( std::vector<float>( 3000, 0.0f ), 1, 48000.0f );
		const Audio a0 = z.convolve( h, false ), a1 = z.convolve( h, true );
		const std::vector<float> & y0 = a0.get_buffer(), & y1 = a1.get_buffer();
		size_t bad = 0;
		for( float v : y0 ) bad += v != 0.0f;
		for( float v : y1 ) bad += !std::isnan( v );
		CHECK( bad == 0 && y1.size() == size_t( 3000 + m ) );
		}
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	null_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		device_checks();
		}
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
