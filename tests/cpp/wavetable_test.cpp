// wavetable_test.cpp -- flan::Wavetable (include/flan/Wavetable.h) over libflan_host.so.
//   wavetable_test --no-device      null sources and bad arguments give null objects; without a device both constructors give a null Wavetable,
//                                   loudly, and synthesize returns a null Audio
//   wavetable_test --device         construction in the three pitch modes from a 0.25 s 220 Hz tone, get_num_waveforms, the table against the
//                                   C ABI bit for bit where the starts are known, synthesis at the tone's own frequency, the four edits, the
//                                   functional constructor
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

static const float SR = 48000.0f;
static const int FRAMES = 12000;                                               // 0.25 s

// 220 Hz with three harmonics, two channels a quarter period apart
static Audio tone()
	{
	std::vector<float> v( 2 * size_t( FRAMES ) );
	for( int c = 0; c < 2; ++c )
		for( int i = 0; i < FRAMES; ++i )
			{
			const double p = 6.283185307179586 * 220.0 * double( i ) / SR + 1.5 * c + 0.3;
			v[size_t( c ) * FRAMES + i] = float( 0.5 * std::sin( p ) + 0.25 * std::sin( 2 * p + 1.1 ) + 0.125 * std::sin( 3 * p + 2.0 ) );
			}
	return Audio::create_from_buffer( std::move( v ), 2, SR );
	}

// the frequency of the largest Hann-windowed DFT bin below 2 kHz, and the bin width
static double peak_hz( const float * x, int n, double * bin_hz )
	{
	*bin_hz = double( SR ) / n;
	double best = -1, best_hz = 0;
	for( int k = 1; k * *bin_hz < 2000.0; ++k )
		{
		double re = 0, im = 0;
		for( int i = 0; i < n; ++i )
			{
			const double w = 0.5 - 0.5 * std::cos( 6.283185307179586 * i / ( n - 1 ) );
			const double a = 6.283185307179586 * double( k ) * i / n;
			re += w * x[i] * std::cos( a ); im -= w * x[i] * std::sin( a );
			}
		const double m = re * re + im * im;
		if( m > best ) { best = m; best_hz = k * *bin_hz; }
		}
	return best_hz;
	}

static void null_checks()
	{
	const Wavetable none;
	CHECK( none.is_null() );
	CHECK( none.synthesize( 1.0f, 220.0f ).is_null() );                          // Wavetable.cpp:275
	CHECK( none.get_num_waveforms( 0 ) == 0 );
	const Wavetable from_null( Audio{} );
	CHECK( from_null.is_null() );                                                // :144
	const Audio a = tone();
	CHECK( Wavetable( a, Wavetable::SnapMode::Zero, Wavetable::PitchMode::None, 2048, .3f, 0 ).is_null() );       // fixed < 1 (:145)
	CHECK( Wavetable( a, Wavetable::SnapMode::Zero, Wavetable::PitchMode::None, 2048, 0.0f, 256 ).is_null() );    // snap_ratio (:146)
	CHECK( Wavetable( a, Wavetable::SnapMode::Zero, Wavetable::PitchMode::None, 2048, .96f, 256 ).is_null() );
	CHECK( Wavetable( []( Second ){ return 0.5f; }, 0, 64 ).is_null() );
	Wavetable edited;
	edited.normalize_in_place(); edited.remove_dc_in_place(); edited.add_fades_in_place( 8 ); edited.remove_jumps_in_place( 8 );      // no-ops on a null
	CHECK( edited.is_null() );
	}

static void no_device_checks()
	{
	const Audio a = tone();
	CHECK( Wavetable( a, Wavetable::SnapMode::Zero, Wavetable::PitchMode::None, 2048, .3f, 218 ).is_null() );
	CHECK( Wavetable( a, Wavetable::SnapMode::Zero, Wavetable::PitchMode::Local ).is_null() );
	CHECK( Wavetable( a, Wavetable::SnapMode::Level, Wavetable::PitchMode::Global ).is_null() );
	const Wavetable f( []( Second t ){ return std::sin( 6.2831853f * t ); }, 4, 64 );
	CHECK( f.is_null() );
	CHECK( f.synthesize( 0.1f, 220.0f ).is_null() );
	}

static void device_checks()
	{
	const Audio a = tone();
	// no pitch tracking, no snapping: starts 0, 218, ... while the next one stays inside the source
	Wavetable fixed( a, Wavetable::SnapMode::None, Wavetable::PitchMode::None, 256, .3f, 218 );
	CHECK( !fixed.is_null() );
	CHECK( fixed.get_num_waveforms( 0 ) == 56 && fixed.get_num_waveforms( 1 ) == 56 );
	CHECK( fixed.get_table().get_num_frames() == 56 * 256 && fixed.get_table().get_num_channels() == 2 );
		{
		std::vector<int32_t> starts;
		for( int c = 0; c < 2; ++c ) for( int k = 0; k < 56; ++k ) starts.push_back( 218 * k );
		const int64_t counts[2] = { 56, 56 };
		std::vector<float> table( 2 * 56 * 256 );
		CHECK( flanhip_wavetable_resample( a.get_sample_pointer( 0, 0 ), 2, FRAMES, starts.data(), counts, 256, table.data(), nullptr, nullptr ) == FLANHIP_OK );
		CHECK( std::memcmp( table.data(), fixed.get_table().get_sample_pointer( 0, 0 ), sizeof( float ) * table.size() ) == 0 );
		bool last_is_zero = true;
		for( int f = 0; f < 256; ++f ) last_is_zero = last_is_zero && table[55 * 256 + f] == 0.0f;
		CHECK( last_is_zero );                                                    // a channel's last slot stays 0, as in the reference
		}

	// the pitch modes: about one waveform per period of 218.2 frames
	Wavetable local( a, Wavetable::SnapMode::Zero, Wavetable::PitchMode::Local, 2048, .3f, 256 );
	Wavetable global( a, Wavetable::SnapMode::Level, Wavetable::PitchMode::Global, 2048, .3f, 256 );
	CHECK( !local.is_null() && !global.is_null() );
	std::printf( "waveforms: local %d / %d, global %d / %d\n", local.get_num_waveforms( 0 ), local.get_num_waveforms( 1 ), global.get_num_waveforms( 0 ),
		global.get_num_waveforms( 1 ) );
	const Audio lp = a.filter_1pole_lowpass( 4000, 2 );
	for( int c = 0; c < 2; ++c )
		{
		CHECK( global.get_num_waveforms( c ) >= 50 && global.get_num_waveforms( c ) <= 57 );
		// Local follows the tracker window by window (a window it cannot read falls back to the global wavelength) and stops where the
		// windows end, 2048 frames before the source does: the count is the C ABI's walk over the same wavelengths
		const std::vector<float> locals = lp.get_local_wavelengths( c, 0, -1, 2048, 128, 1, 32 );
		const Frame average = Frame( lp.get_average_wavelength( locals, .2f, 64 ) );
		int64_t count = 0;
		CHECK( flanhip_wavetable_starts( a.get_sample_pointer( c, 0 ), FRAMES, locals.data(), int64_t( locals.size() ), average, FLANHIP_WAVETABLE_SNAP_ZERO,
			FLANHIP_WAVETABLE_PITCH_LOCAL, .3f, 256, nullptr, nullptr, 0, &count ) == FLANHIP_OK );
		CHECK( local.get_num_waveforms( c ) == count && count >= 20 && count <= 57 );
		}
	CHECK( local.get_table().get_num_frames() % 2048 == 0 );

	// synthesis at the tone's own frequency: the spectrum's peak within one bin of 220 Hz
	for( const Wavetable * wt : { &fixed, &local, &global } )
		{
		const Audio y = wt->synthesize( 0.25f, 220.0f, []( Second t ){ return 0.2f + 2.0f * t; }, true );
		CHECK( !y.is_null() && y.get_num_frames() == FRAMES && y.get_num_channels() == 2 );
		if( y.is_null() ) continue;
		for( int c = 0; c < 2; ++c )
			{
			double bin = 0;
			const double hz = peak_hz( y.get_sample_pointer( c, 0 ), FRAMES, &bin );
			std::printf( "synthesis: channel %d peaks at %.1f Hz (bin width %.1f Hz)\n", c, hz, bin );
			CHECK( std::fabs( hz - 220.0 ) <= bin );
			}
		}
	CHECK( fixed.synthesize( 0.0f, 220.0f ).is_null() );                          // no frames
	CHECK( fixed.synthesize( 0.1f, 220.0f, 0, true, 0.0f ).is_null() );           // a granularity below one frame
	const Audio swept = fixed.synthesize( 0.1f, []( Second t ){ return 110.0f + 2000.0f * t; }, 0.5f, false );
	CHECK( !swept.is_null() && swept.get_num_frames() == 4800 );

	// the edits
	const int W = 256, slots = 56;
	auto slot = [&]( const Wavetable & w, int c, int k ) { return w.get_table().get_sample_pointer( c, k * W ); };
	fixed.remove_dc_in_place();
	for( int k : { 0, 17, 54 } )
		{
		double sum = 0;
		for( int f = 0; f < W; ++f ) sum += slot( fixed, 1, k )[f];
		CHECK( std::fabs( sum / W ) < 1e-6 );
		}
	fixed.normalize_in_place();
	for( int k : { 0, 17, 54 } )
		{
		float m = 0;
		for( int f = 0; f < W; ++f ) m = std::max( m, std::fabs( slot( fixed, 0, k )[f] ) );
		CHECK( m == 1.0f );
		}
	const float before_first = slot( fixed, 0, 3 )[0], before_mid = slot( fixed, 0, 3 )[W / 2];
	fixed.add_fades_in_place( 32 );
	CHECK( std::fabs( slot( fixed, 0, 3 )[0] - before_first * std::sin( 3.14159265f / 2.0f / 32.0f ) ) <= 1e-6f * std::fabs( before_first ) );
	CHECK( slot( fixed, 0, 3 )[W / 2] == before_mid );
	fixed.remove_jumps_in_place( 32 );
	CHECK( std::fabs( slot( fixed, 0, 3 )[0] - slot( fixed, 0, 3 )[W - 1] ) < 0.1f * std::fabs( before_mid ) + 1e-3f );
	bool finite = true, last_zero = true;
	for( int i = 0; i < 2 * slots * W; ++i ) finite = finite && std::isfinite( fixed.get_table().get_sample_pointer( 0, 0 )[i] );
	for( int f = 0; f < W; ++f ) last_zero = last_zero && slot( fixed, 0, slots - 1 )[f] == 0.0f;
	CHECK( finite && last_zero );
	CHECK( !fixed.synthesize( 0.05f, 220.0f ).is_null() );                        // the edited table still plays

	// the functional constructor: wave k in slot k
	const Wavetable fn( []( Second t ){ return std::sin( 6.2831853f * t ) * ( 1.0f + std::floor( t ) ); }, 3, 64 );
	CHECK( !fn.is_null() && fn.get_num_waveforms( 0 ) == 3 && fn.get_table().get_num_frames() == 3 * 64 );
	bool exact = true;
	for( int k = 0; k < 3; ++k ) for( int f = 0; f < 64; ++f )
		{
		const float t = k + float( f ) / 64;
		exact = exact && fn.get_table().get_sample_pointer( 0, 0 )[k * 64 + f] == std::sin( 6.2831853f * t ) * ( 1.0f + std::floor( t ) );
		}
	CHECK( exact );
	const Audio y = fn.synthesize( 0.1f, 750.0f, []( Second t ){ return 5.0f * t; } );
	CHECK( !y.is_null() && y.get_num_frames() == 4800 && y.get_num_channels() == 1 );
	}

int main( int argc, char ** argv )
	{
	const bool device = argc > 1 && std::strcmp( argv[1], "--device" ) == 0;
	null_checks();
	if( device )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		device_checks();
		}
	else if( flanhip_device_count() < 1 ) no_device_checks();
	if( failures ) { std::printf( "%d checks FAILED\n", failures ); return 1; }
	std::printf( "PASSED\n" );
	return 0;
	}
