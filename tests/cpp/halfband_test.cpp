// halfband_test.cpp -- Audio::halfband_modulate, shift_frequency and halfband_multiply (include/flan/Audio.h) over libflan_host.so.
//   halfband_test --no-device  null in, null out for all three; without a device the C ABI answers FLANHIP_ERR_NO_DEVICE and every method
//                              fails loudly with a null result
//   halfband_test --device     each method with constants and with callables against the C ABI's host forms fed what the method computes
//                              on the host -- the sampled modulator; the cutoff curves and the summed phase of a shift -- bit for bit
#include <algorithm>
#include <cmath>
#include <complex>
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

static bool same_bits( const void * a, const void * b, size_t bytes ) { return std::memcmp( a, b, bytes ) == 0; }
static bool same_audio( const Audio & a, const std::vector<float> & want )
	{
	return !a.is_null() && a.get_buffer().size() == want.size() && same_bits( a.get_buffer().data(), want.data(), sizeof( float ) * want.size() );
	}

static std::vector<float> noise( size_t n, uint32_t seed )
	{
	std::vector<float> v( n );
	for( size_t i = 0; i < n; ++i ) { seed = seed * 1664525u + 1013904223u; v[i] = float( int32_t( seed >> 8 ) - ( 1 << 23 ) ) / float( 1 << 24 ); }
	return v;
	}

static const auto phasor = []( Second t ){ return std::complex<float>( 0.9f * std::cos( 1900.0f * t ), 0.7f * std::sin( 1100.0f * t ) ); };
static const auto wander = []( Second t ){ return 300.0f * std::sin( 25.0f * t + 1.0f ); };     // through 0 several times in 9001 frames

static void null_checks()
	{
	std::ostringstream captured;                                               // "Null Audio created"
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	const Audio some = Audio::create_empty_with_frames( 100 );
	CHECK( Audio().halfband_modulate( std::complex<float>( 1.0f, 0.0f ) ).is_null() );
	CHECK( Audio().halfband_modulate( phasor ).is_null() );
	CHECK( Audio().shift_frequency( 250.0f ).is_null() );
	CHECK( Audio().shift_frequency( wander, 50.0f ).is_null() );
	CHECK( Audio().halfband_multiply( some ).is_null() );
	CHECK( some.halfband_multiply( Audio() ).is_null() );
	CHECK( Audio().halfband_multiply( Audio() ).is_null() );
	std::cout.rdbuf( old );
	CHECK( captured.str().find( "Null Audio created" ) != std::string::npos );
	}

static void no_device_checks()
	{
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 40 );           // never dereferenced
	const float * p = static_cast<const float*>( bogus );
	float * q = static_cast<float*>( bogus ) + 4096;
	CHECK( flanhip_hilbert_dev( p, 2, 1000, 48000.0f, q, q + 4096, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_halfband_modulate_dev( p, 2, 1000, 48000.0f, nullptr, 1.0f, nullptr, 0.0f, nullptr, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_halfband_multiply_dev( p, 2, 1000, 48000.0f, p, 1, 900, 44100.0f, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const std::vector<float> x = noise( 2 * 1000, 1 );
	std::vector<float> out( x.size() );
	CHECK( flanhip_halfband_modulate( x.data(), 2, 1000, 48000.0f, nullptr, 1.0f, nullptr, 0.0f, nullptr, out.data(), nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );
	std::ostringstream captured;
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	int sampled = 0;
	CHECK( a.halfband_modulate( std::complex<float>( 0.5f, 0.5f ) ).is_null() );
	CHECK( a.halfband_modulate( phasor ).is_null() );
	CHECK( a.shift_frequency( 250.0f ).is_null() );
	CHECK( a.shift_frequency( Function<Second, Frequency>( [&]( Second ){ ++sampled; return 100.0f; }, ExecutionPolicy::Linear_Sequenced ) ).is_null() );
	CHECK( a.halfband_multiply( a ).is_null() );
	std::cout.rdbuf( old );
	CHECK( sampled == 0 );                                                     // without a device nothing is sampled
	CHECK( !a.is_null() && same_bits( a.get_buffer().data(), x.data(), sizeof( float ) * x.size() ) );
	}

static void device_checks()
	{
	const Channel ch = 2;
	const Frame n = 9001;
	const float sr = 48000.0f;
	const size_t N = size_t( n );
	const std::vector<float> x = noise( size_t( ch ) * n, 7 );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, sr );
	std::vector<float> want( x.size() ), stage( x.size() );
	const float step = 1.0f / sr;

	// halfband_modulate: a constant goes as two scalars, a callable as two curves sampled at f * ( 1.0f / sr ); the result stays in HBM until read
		{
		const Audio y = a.halfband_modulate( std::complex<float>( 0.6f, -0.8f ) );
		CHECK( !y.is_null() && y.is_device_resident() && !y.host_copy_is_current() );
		CHECK( y.get_num_channels() == ch && y.get_num_frames() == n && y.get_sample_rate() == sr );
		CHECK( flanhip_halfband_modulate( x.data(), ch, n, sr, nullptr, 0.6f, nullptr, -0.8f, nullptr, want.data(), nullptr ) == FLANHIP_OK && same_audio( y, want ) );
		CHECK( !same_bits( want.data(), x.data(), sizeof( float ) * want.size() ) );
		std::vector<float> re( N ), im( N );
		for( Frame f = 0; f < n; ++f ) { const std::complex<float> m = phasor( f * step ); re[size_t( f )] = m.real(); im[size_t( f )] = m.imag(); }
		CHECK( flanhip_halfband_modulate( x.data(), ch, n, sr, re.data(), 0.0f, im.data(), 0.0f, nullptr, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.halfband_modulate( phasor ), want ) );
		}

	// shift_frequency: the two order-8 filters with the cutoffs the shift moves, then the modulation by the phase summed in fp32
	auto shifted = [&]( const std::vector<float> & s, float low_cutoff, std::vector<float> & out )
		{
		const float high_cutoff = sr / 2 - 1000;
		std::vector<float> lp( N ), hp( N ), phase( N );
		float sum = 0.0f;
		for( size_t f = 0; f < N; ++f )
			{
			lp[f] = s[f] > 0 ? high_cutoff - s[f] : high_cutoff;
			hp[f] = s[f] < 0 ? low_cutoff - s[f] : low_cutoff;
			phase[f] = sum;
			sum = sum + s[f] * pi2 / sr;
			}
		return flanhip_filter_1pole( x.data(), ch, n, sr, lp.data(), 0.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 8, stage.data(), nullptr ) == FLANHIP_OK
			&& flanhip_filter_1pole( stage.data(), ch, n, sr, hp.data(), 0.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 8, stage.data(), nullptr ) == FLANHIP_OK
			&& flanhip_halfband_modulate( stage.data(), ch, n, sr, nullptr, 0.0f, nullptr, 0.0f, phase.data(), out.data(), nullptr ) == FLANHIP_OK;
		};
		{
		std::vector<float> s( N );
		bool up = false, down = false;
		for( Frame f = 0; f < n; ++f ) { s[size_t( f )] = wander( f * step ); up = up || s[size_t( f )] > 200; down = down || s[size_t( f )] < -200; }
		CHECK( up && down );
		CHECK( shifted( s, 30.0f, want ) );
		const Audio y = a.shift_frequency( wander );
		CHECK( !y.is_null() && y.is_device_resident() && y.get_num_frames() == n && y.get_sample_rate() == sr );
		CHECK( same_audio( y, want ) );
		CHECK( shifted( s, 80.0f, want ) && same_audio( a.shift_frequency( wander, 80.0f ), want ) );
		// a constant samples nothing and equals the callable that returns it
		std::fill( s.begin(), s.end(), -120.0f );
		CHECK( shifted( s, 30.0f, want ) && same_audio( a.shift_frequency( -120.0f ), want ) );
		CHECK( same_audio( a.shift_frequency( []( Second ){ return -120.0f; } ), want ) );
		}

	// halfband_multiply: each operand through its own band-pass and the network at its own sample rate; the channels and frames both have
		{
		const Channel ch_b = 1;
		const Frame n_b = 7000;
		const float sr_b = 44100.0f;
		const std::vector<float> xb = noise( size_t( ch_b ) * n_b, 11 );
		const Audio b = Audio::create_from_buffer( std::vector<float>( xb ), ch_b, sr_b );
		std::vector<float> fa( x.size() ), fb( xb.size() ), out( size_t( ch_b ) * n_b );
		CHECK( flanhip_filter_1pole( x.data(), ch, n, sr, nullptr, sr / 2 - 2000, FLANHIP_FILTER_BUTTERWORTH_LOW, 8, fa.data(), nullptr ) == FLANHIP_OK );
		CHECK( flanhip_filter_1pole( fa.data(), ch, n, sr, nullptr, 30.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 8, fa.data(), nullptr ) == FLANHIP_OK );
		CHECK( flanhip_filter_1pole( xb.data(), ch_b, n_b, sr_b, nullptr, sr_b / 2 - 2000, FLANHIP_FILTER_BUTTERWORTH_LOW, 8, fb.data(), nullptr ) == FLANHIP_OK );
		CHECK( flanhip_filter_1pole( fb.data(), ch_b, n_b, sr_b, nullptr, 30.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 8, fb.data(), nullptr ) == FLANHIP_OK );
		CHECK( flanhip_halfband_multiply( fa.data(), ch, n, sr, fb.data(), ch_b, n_b, sr_b, out.data(), nullptr ) == FLANHIP_OK );
		const Audio y = a.halfband_multiply( b );
		CHECK( !y.is_null() && y.is_device_resident() );
		CHECK( y.get_num_channels() == ch_b && y.get_num_frames() == n_b && y.get_sample_rate() == sr );
		CHECK( same_audio( y, out ) );
		// the other way round the same samples (the product commutes bit for bit), at the other operand's sample rate
		const Audio z = b.halfband_multiply( a );
		CHECK( !z.is_null() && z.get_sample_rate() == sr_b && same_audio( z, out ) );
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
