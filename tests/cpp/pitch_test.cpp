// pitch_test.cpp -- Audio::get_local_wavelength(s), get_average_wavelength, get_local_frequency / frequencies and get_frequency_envelope
// (include/flan/Audio.h) over libflan_host.so.
//   pitch_test --no-device          a null Audio's answers; without a device the C ABI answers FLANHIP_ERR_NO_DEVICE and the methods fail loudly
//                                   with empty answers; what needs no device (the average, no window at all) works
//   pitch_test --device             the methods against the C ABI's host form on the same samples, bit for bit
//   pitch_test --dump IN OUT        IN: raw fp32 samples of one channel at 48 kHz; OUT: what the methods answer, as text, for the Python suite
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

#include "flan/flan.h"
#include "flanhip.h"

using namespace flan;

static int failures = 0;
#define CHECK( cond ) do { if( !( cond ) ) { std::printf( "FAILED: %s (line %d)\n", #cond, __LINE__ ); ++failures; } } while( 0 )

static bool same_bits( const std::vector<float> & a, const std::vector<float> & b )
	{
	return a.size() == b.size() && std::memcmp( a.data(), b.data(), sizeof( float ) * a.size() ) == 0;
	}

// a tone of `period` frames with three harmonics over a noise floor
static std::vector<float> tone( size_t n, float period, uint32_t seed )
	{
	std::vector<float> v( n );
	for( size_t i = 0; i < n; ++i )
		{
		seed = seed * 1664525u + 1013904223u;
		const float noise = float( int32_t( seed >> 8 ) - ( 1 << 23 ) ) / float( 1 << 23 );
		const double p = 6.283185307179586 * double( i ) / period;
		v[i] = float( 0.3 * std::sin( p ) + 0.15 * std::sin( 2 * p + 1 ) + 0.1 * std::sin( 3 * p + 2 ) ) + 0.02f * noise;
		}
	return v;
	}

static void null_checks()
	{
	const Audio none;
	CHECK( none.get_local_wavelength( 0, 0 ) == 0 );                              // AudioInformation.cpp:140
	CHECK( none.get_local_wavelengths( 0 ).empty() );                             // :178
	CHECK( none.get_average_wavelength( 0 ) == 0 );                               // :241
	CHECK( none.get_average_wavelength( std::vector<float>{ 100, 200 } ) == 0 );  // :251
	CHECK( none.get_local_frequencies( 0 ).empty() );
	CHECK( std::isinf( none.get_local_frequency( 0 ) ) || std::isnan( none.get_local_frequency( 0 ) ) );     // :270: a null Audio's rate over 0
	const auto envelope = none.get_frequency_envelope();
	CHECK( envelope( 0.0f ) == 0 && envelope( 0.1f ) == 0 );
	}

// the host-only parts, with or without a device
static void host_only_checks( const Audio & a )
	{
	CHECK( a.get_average_wavelength( std::vector<float>{ 100, 0, 102, 0 } ) == 101.0f );
	CHECK( a.get_average_wavelength( std::vector<float>{ 100, 0, 102, -1 } ) == 67.0f );                     // a -1 is averaged in
	CHECK( a.get_average_wavelength( std::vector<float>{ -1, -1, 100 }, 0.5f ) == -1.0f );
	CHECK( a.get_average_wavelength( std::vector<float>{ 100, 104 }, 0, 1.9f ) == -1.0f );
	CHECK( a.get_average_wavelength( std::vector<float>{ 100, 104 }, 0, 2.0f ) == 102.0f );
	CHECK( a.get_average_wavelength( std::vector<float>{} ) == -1.0f );
	// no window at all: nothing to launch
	CHECK( a.get_local_wavelengths( 0, 0, -1, a.get_num_frames(), 128 ).empty() );
	CHECK( a.get_local_wavelengths( 0, 100, 50 ).empty() );
	}

static void no_device_checks()
	{
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 40 );               // never dereferenced
	const float * p = static_cast<const float*>( bogus );
	float * q = static_cast<float*>( bogus ) + ( 1 << 20 );
	CHECK( flanhip_audio_local_wavelengths_dev( p, 8000, 0, -1, 2048, 128, 0.2f, 10, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_local_wavelength_dev( p, 2048, 0.2f, 10, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const std::vector<float> x = tone( 8000, 218.0f, 1 );
	std::vector<float> out( 64 );
	CHECK( flanhip_audio_local_wavelengths( x.data(), 8000, 48000.0f, 0, -1, 2048, 128, 0.2f, 10, out.data(), nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 1, 48000.0f );
	CHECK( a.get_local_wavelengths( 0 ).empty() );
	CHECK( a.get_local_wavelength( 0, 0 ) == 0 );
	CHECK( a.get_local_frequencies( 0 ).empty() );
	CHECK( a.get_average_wavelength( 0 ) == -1.0f );                              // of an empty vector
	CHECK( a.get_frequency_envelope()( 0.05f ) == 0 );
	host_only_checks( a );
	}

static void device_checks()
	{
	const Frame n = 9001;
	const float sr = 48000.0f;
	std::vector<float> x = tone( size_t( n ), 218.18f, 7 );
	const std::vector<float> y = tone( size_t( n ), 97.3f, 8 );
	x.insert( x.end(), y.begin(), y.end() );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 2, sr );
	host_only_checks( a );

	for( Channel channel = 0; channel < 2; ++channel )
		{
		const float * row = x.data() + size_t( channel ) * size_t( n );
		// the defaults: ( 0, -1, 2048, 128, 0.2f, 10 )
		std::vector<float> want( size_t( flanhip_audio_local_wavelengths_count( n, 0, -1, 2048, 128 ) ) );
		CHECK( want.size() == 55 );
		CHECK( flanhip_audio_local_wavelengths( row, n, sr, 0, -1, 2048, 128, 0.2f, 10, want.data(), nullptr ) == FLANHIP_OK );
		const std::vector<float> w = a.get_local_wavelengths( channel );
		CHECK( same_bits( w, want ) );
		int found = 0;
		for( float v : w ) found += v != 0;
		CHECK( found > 40 );                                                       // the tones are there to be found
		// frequencies: the rate over every non-zero wavelength
		std::vector<float> f = want;
		for( float & v : f ) if( v != 0 ) v = sr / v;
		CHECK( same_bits( a.get_local_frequencies( channel ), f ) );
		// the average of the vector and of the channel
		float mean = 0;
		CHECK( flanhip_average_wavelength( want.data(), int64_t( want.size() ), 0.0f, -1.0f, &mean ) == FLANHIP_OK );
		CHECK( a.get_average_wavelength( w ) == mean && a.get_average_wavelength( channel ) == mean );
		CHECK( std::fabs( mean - ( channel == 0 ? 218.18f : 97.3f ) ) < 1.0f );  // the tones' periods
		// other arguments
		want.assign( size_t( flanhip_audio_local_wavelengths_count( n, 301, 7000, 500, 77 ) ), 0.0f );
		CHECK( flanhip_audio_local_wavelengths( row, n, sr, 301, 7000, 500, 77, 0.35f, 25, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_bits( a.get_local_wavelengths( channel, 301, 7000, 500, 77, 0.35f, 25 ), want ) );
		// one window: the raw value of that window (no continuity pass), also the last window that fits
		for( Frame start : { Frame( 0 ), Frame( 1280 ), n - 2048 } )
			{
			if( start + 2049 > n ) continue;                                       // (the host form wants one frame more than the window)
			float one = -1;
			CHECK( flanhip_audio_local_wavelengths( row + start, 2049, sr, 0, -1, 2048, 4096, 0.2f, 10, &one, nullptr ) == FLANHIP_OK );
			const float got = a.get_local_wavelength( channel, start );
			CHECK( std::memcmp( &got, &one, sizeof( float ) ) == 0 );
			const float freq = a.get_local_frequency( channel, start );
			CHECK( freq == sr / got );
			}
		CHECK( a.get_local_wavelength( channel, n - 2048 ) > 0 );
		}
	// what lies outside the signal is refused, loudly
	CHECK( a.get_local_wavelength( 2, 0 ) == 0 && a.get_local_wavelength( 0, n - 2047 ) == 0 && a.get_local_wavelength( 0, -1 ) == 0 );
	CHECK( a.get_local_wavelengths( 2 ).empty() && a.get_local_wavelengths( 0, 0, n + 1 ).empty() && a.get_local_wavelengths( 0, 0, -1, 2048, 0 ).empty() );
	CHECK( a.get_local_wavelengths( 0, 0, -1, 16386, 128 ).empty() );
	// a raised canceller
	std::atomic<bool> stop( true );
	CHECK( a.get_local_wavelengths( 0, 0, -1, 2048, 128, 0.2f, 10, stop ).empty() );
	// the envelope: linear between the hops of the mono mix's frequencies, 0 outside them
	const Audio mono = a.convert_to_mono();
	const std::vector<float> f = mono.get_local_frequencies( 0 );
	const auto envelope = a.get_frequency_envelope();
	CHECK( f.size() == 55 );
	for( int k = 0; k < 50 && f.size() == 55; ++k )
		{
		const float t = ( k + 0.37f ) * ( 56.0f * 128.0f / sr ) / 50.0f;
		const float xk = t * sr / 128;
		float want = 0;
		if( 0 <= xk && xk < 54 ) { const Frame x1 = Frame( std::floor( xk ) ); want = f[x1] + ( f[x1 + 1] - f[x1] ) * ( xk - x1 ); }
		const float got = envelope( t );
		CHECK( std::memcmp( &got, &want, sizeof( float ) ) == 0 );
		}
	CHECK( envelope( -0.001f ) == 0 );
	}

static std::string row_text( const char * name, const std::vector<float> & v )
	{
	std::ostringstream s;
	s << name;
	char buffer[32];
	for( float f : v ) { std::snprintf( buffer, sizeof buffer, " %.9g", f ); s << buffer; }
	s << "\n";
	return s.str();
	}

static int dump( const char * in_path, const char * out_path )
	{
	std::FILE * in = std::fopen( in_path, "rb" );
	if( !in ) { std::printf( "FAILED: cannot read %s\n", in_path ); return 1; }
	std::vector<float> x;
	float block[4096];
	for( size_t got; ( got = std::fread( block, sizeof( float ), 4096, in ) ) > 0; ) x.insert( x.end(), block, block + got );
	std::fclose( in );
	const Frame n = Frame( x.size() );
	const Audio a = Audio::create_from_buffer( std::move( x ), 1, 48000.0f );
	std::string text;
	const std::vector<float> w = a.get_local_wavelengths( 0 );
	text += row_text( "wavelengths", w );
	text += row_text( "frequencies", a.get_local_frequencies( 0 ) );
	text += row_text( "average", { a.get_average_wavelength( w ), a.get_average_wavelength( 0 ), a.get_average_wavelength( w, 0, 1.0f ) } );
	std::vector<float> single;
	for( Frame start : { Frame( 0 ), Frame( 640 ), n - 2048 } ) { single.push_back( a.get_local_wavelength( 0, start ) ); single.push_back( a.get_local_frequency( 0, start ) ); }
	text += row_text( "single", single );
	const auto envelope = a.get_frequency_envelope();
	std::vector<float> times, values;
	for( int k = 0; k < 50; ++k )
		{
		times.push_back( ( k + 0.37f ) * ( float( w.size() + 1 ) * 128.0f / 48000.0f ) / 50.0f );            // the last ones lie behind the last hop
		values.push_back( envelope( times.back() ) );
		}
	text += row_text( "times", times );
	text += row_text( "envelope", values );
	std::FILE * out = std::fopen( out_path, "w" );
	if( !out ) { std::printf( "FAILED: cannot write %s\n", out_path ); return 1; }
	std::fputs( text.c_str(), out );
	std::fclose( out );
	return 0;
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	std::ostringstream captured;                                               // "Null Audio created"
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	null_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) || !std::strcmp( mode, "--dump" ) )
		{
		if( flanhip_device_count() < 1 ) { std::cout.rdbuf( old ); std::printf( "FAILED: no device\n" ); return 1; }
		if( !std::strcmp( mode, "--device" ) ) device_checks();
		else if( argc < 4 || dump( argv[2], argv[3] ) ) ++failures;
		}
	std::cout.rdbuf( old );
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
