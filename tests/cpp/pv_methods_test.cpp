// pv_methods_test.cpp -- every flan::PV frame processor through the C++ surface, its whole output written out for
// tests/test_gpu_pv_methods_cpp.py to hold to the oracle (the case table and the NumPy twins of the callables below are in
// tests/pv_methods_reference.py; a case carries the same name on both sides).
//
//   --run IN_DIR OUT_DIR     needs the device: reads A.pv, X.pv, B.pv, BIG.pv, runs the cases, writes one file per result
//   --sample-only OUT_DIR    no device: what the callables give through the host calls PV.cpp makes
//
// File format: int32 channels, frames, bins, window; float32 sample_rate, analysis_rate; the MF pairs as float32.  A null result is a
// zero header; audio has bins = 0 and the samples as float32 [channel][frame].  A --sample-only dump is int32 element kind (0 float32,
// 1 int32, 2 uint32), int32 count, the elements.
//
// The driver compares nothing itself but this: the input's bits (host copy and device copy) after every case, and the result of every
// data-dependent method on a device-only PV against the result on a PV whose host copy is current.
//
// The callables use + - * /, comparisons and selects on floats only (build with -ffp-contract=off), so NumPy reproduces them to the bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "flan/Audio.h"
#include "flan/PV.h"
#include "flanhip.h"

using namespace flan;

namespace {

// ---- the callables --------------------------------------------------------------------------------------------------------------------
const auto mt_mono    = []( TF a ){ return a.t * 1.5f + ( a.f > 8000.0f ? 0.01f : 0.0f ); };
const auto mt_back    = []( TF a ){ return a.f < 6000.0f ? a.t * 1.25f : 0.06f - a.t * 0.5f; };
const auto mt_lastmax = []( TF a ){ return a.t * 0.75f + a.f * 2e-6f; };
const auto mt_big     = []( TF a ){ return a.t * 0.5f + a.f * 1e-5f; };
const auto st_tf      = []( TF a ){ return 1.0f + a.t * 4.0f + a.f * 2e-5f; };
const auto st_big     = []( TF a ){ return 0.5f + a.t * 0.05f + a.f * 1e-5f; };
const auto mfq        = []( TF a ){ return a.f * ( 1.0f + a.t * 2.0f ) + 20.0f; };
const auto mfq_big    = []( TF a ){ return a.f * ( 1.0f + a.t * 0.02f ) + 20.0f; };
const auto rp         = []( TF a ){ return 1.0f + a.t * 2.0f + a.f * 1e-5f; };
const auto amt        = []( TF a ){ return a.t * 20.0f - 0.3f + a.f * 2e-5f; };
const auto dc         = []( TF a ){ return a.t < 0.07f ? 0.6f + a.f * 4e-5f : 1.1f - a.t * 4.0f - a.f * 5e-5f; };
const auto ds         = []( TF a ){ return 1.0f + a.t * 30.0f + a.f * 1e-4f; };
const auto sm         = []( TF a ){ return 0.01f + a.t * 0.2f + a.f * 5e-7f; };
const auto gr         = []( TF a ){ return int( 1.0f + a.t * 40.0f + a.f * 1e-4f ); };
const auto sel        = []( TF a ){ return TF{ 0.09f - a.t * 0.8f + a.f * 1e-6f, a.f * 1.1f - 300.0f + a.t * 1000.0f }; };
const auto md         = []( TF a ){ return TF{ a.t * 1.3f + 0.0007f + a.f * 1e-7f, a.f * 1.05f + 37.0f + a.t * 100.0f }; };
const auto md_long    = []( TF a ){ return TF{ a.t * 10000.0f, a.f }; };
const auto nl         = []( Second t ){ return Bin( t * 4000.0f - 20.0f ); };
const auto sp         = []( Second t ){ return t < 0.01f ? -2.0f : ( t < 0.02f ? 0.5f : ( t > 0.0501f && t < 0.0529f ? 40.0f : 1.0f + t * 30.0f ) ); };
const auto dist_rat   = []( Second t ){ return 1.0f - t * t; };
const auto hs         = []( std::pair<Second, Harmonic> p ){ return ( 1.0f - p.first * 5.0f ) / ( 1.0f + float( p.second ) ); };
const auto shaper     = []( MF mf ){ return MF{ mf.m * 0.5f + 0.001f, mf.f * 1.02f + 10.0f }; };
const float c_mt = 0.05f, c_mfq = 1000.0f, c_rp = 1.5f, c_amt = 0.5f, c_dc = 0.5f, c_ds = 3.0f, c_sm = 0.02f, c_sp = 2.5f, c_hs = 0.5f;
const int c_gr = 3, c_nl = 10;
const TF c_sel{ 0.03f, 5000.0f }, c_md{ 0.05f, 3000.0f };

// ---- files ----------------------------------------------------------------------------------------------------------------------------
struct Header { int32_t channels, frames, bins, window; float sample_rate, analysis_rate; };
static_assert( sizeof( Header ) == 24 && sizeof( MF ) == 8 && sizeof( TF ) == 8, "packed" );

int failures = 0;
void fail( const std::string & what ) { ++failures; std::printf( "FAIL %s\n", what.c_str() ); }

PVBuffer::Format format_of( const std::string & name )
	{
	PVBuffer::Format f;
	if( name == "A" )   { f.num_channels = 2; f.num_frames = 61;   f.num_bins = 129;  f.window_size = 256;  f.sample_rate = 48000; f.analysis_rate = 750; }
	if( name == "X" )   { f.num_channels = 2; f.num_frames = 53;   f.num_bins = 101;  f.window_size = 200;  f.sample_rate = 44100; f.analysis_rate = 441; }
	if( name == "B" )   { f.num_channels = 1; f.num_frames = 40;   f.num_bins = 65;   f.window_size = 128;  f.sample_rate = 48000; f.analysis_rate = 750; }
	if( name == "BIG" ) { f.num_channels = 1; f.num_frames = 1100; f.num_bins = 1025; f.window_size = 2048; f.sample_rate = 48000; f.analysis_rate = 93.75f; }
	return f;
	}

bool write_file( const std::string & path, const void * head, size_t head_bytes, const void * body, size_t body_bytes )
	{
	std::FILE * fh = std::fopen( path.c_str(), "wb" );
	if( !fh ) { fail( "cannot write " + path ); return false; }
	bool ok = std::fwrite( head, 1, head_bytes, fh ) == head_bytes;
	if( body_bytes ) ok = std::fwrite( body, 1, body_bytes, fh ) == body_bytes && ok;
	ok = std::fclose( fh ) == 0 && ok;
	if( !ok ) fail( "short write " + path );
	return ok;
	}

PV read_pv( const std::string & dir, const std::string & name )
	{
	const std::string path = dir + "/" + name + ".pv";
	std::FILE * fh = std::fopen( path.c_str(), "rb" );
	if( !fh ) { fail( "cannot read " + path ); return PV(); }
	Header h{};
	const PVBuffer::Format want = format_of( name );
	if( std::fread( &h, sizeof( h ), 1, fh ) != 1 || h.channels != want.num_channels || h.frames != want.num_frames || h.bins != want.num_bins || h.window != want.window_size
			|| h.sample_rate != want.sample_rate || h.analysis_rate != want.analysis_rate )
		{ std::fclose( fh ); fail( "format of " + path ); return PV(); }
	PV pv = PV::create_from_format( want );
	std::vector<MF> & buffer = pv.get_buffer();
	if( std::fread( buffer.data(), sizeof( MF ), buffer.size(), fh ) != buffer.size() ) fail( "short read " + path );
	std::fclose( fh );
	return pv;
	}

struct Runner
	{
	std::string out_dir;
	const PV * input = nullptr;             // its bits are checked after every case
	std::vector<MF> saved;

	void begin( const PV & in ) { input = &in; saved = std::as_const( in ).get_buffer(); }

	void check_input( const std::string & name )
		{
		if( !input ) return;
		const size_t bytes = sizeof( MF ) * saved.size();
		if( std::as_const( *input ).get_buffer().size() != saved.size() || std::memcmp( std::as_const( *input ).get_buffer().data(), saved.data(), bytes ) != 0 )
			fail( name + ": the input's host copy changed" );
		std::vector<MF> back( saved.size() );
		const MF * d = input->device_data();
		if( !d || flanhip_memcpy_d2h( back.data(), d, bytes, nullptr ) != FLANHIP_OK || flanhip_stream_synchronize( nullptr ) != FLANHIP_OK )
			fail( name + ": the input's device copy could not be read" );
		else if( std::memcmp( back.data(), saved.data(), bytes ) != 0 ) fail( name + ": the input's device copy changed" );
		}

	void write( const std::string & name, const PV & r )
		{
		Header h{};
		if( r.is_null() ) { write_file( out_dir + "/" + name + ".pv", &h, sizeof( h ), nullptr, 0 ); return; }
		h = Header{ r.get_num_channels(), r.get_num_frames(), r.get_num_bins(), r.get_window_size(), r.get_sample_rate(), r.get_analysis_rate() };
		const std::vector<MF> & b = std::as_const( r ).get_buffer();
		write_file( out_dir + "/" + name + ".pv", &h, sizeof( h ), b.data(), sizeof( MF ) * b.size() );
		}

	void put( const std::string & name, const PV & r )
		{
		write( name, r );
		check_input( name );
		if( r.is_null() ) std::printf( "case %s: null\n", name.c_str() );
		else std::printf( "case %s: %d x %d x %d\n", name.c_str(), int( r.get_num_channels() ), int( r.get_num_frames() ), int( r.get_num_bins() ) );
		std::fflush( stdout );
		}

	// convert_to_audio of `source` first (a result straight from stretch / shape carries its synthesis workspace), then source's own bits
	void put_audio( const std::string & name, const PV & source )
		{
		const Audio a = source.convert_to_audio();
		Header h{};
		if( !a.is_null() )
			{
			h = Header{ a.get_num_channels(), a.get_num_frames(), 0, 0, a.get_sample_rate(), 0.0f };
			const std::vector<float> & b = a.get_buffer();
			write_file( out_dir + "/" + name + ".pv", &h, sizeof( h ), b.data(), sizeof( float ) * b.size() );
			}
		else write_file( out_dir + "/" + name + ".pv", &h, sizeof( h ), nullptr, 0 );
		check_input( name );
		std::printf( "case %s: %s %d x %d\n", name.c_str(), a.is_null() ? "null" : "audio", int( h.channels ), int( h.frames ) );
		std::fflush( stdout );
		}

	// a data-dependent method on a PV whose host copy is current, then on a device-only PV with the same bits: two cases, and the same bits required
	template<typename Method>
	void put_both( const std::string & name, const PV & in, const Method & method, const std::string & audio_name = "" )
		{
		const PV on_host = method( in );
		if( !audio_name.empty() ) put_audio( audio_name, on_host );
		put( name, on_host );
		const PV dev = PV::join( std::vector<const PV *>{ &in } );                     // the same bits, in HBM only
		if( dev.is_null() || dev.host_copy_is_current() ) fail( name + ": no device-only copy" );
		const PV from_dev = method( dev );
		if( dev.host_copy_is_current() ) fail( name + ": the method brought the device-only PV to the host" );
		const size_t dot = name.rfind( '.' );                                          // "method.variant.INPUT" -> "method.variant_device_only.INPUT"
		put( name.substr( 0, dot ) + "_device_only" + name.substr( dot ), from_dev );
		const std::vector<MF> & a = std::as_const( on_host ).get_buffer();
		const std::vector<MF> & b = std::as_const( from_dev ).get_buffer();
		if( on_host.is_null() != from_dev.is_null() || a.size() != b.size() || std::memcmp( a.data(), b.data(), sizeof( MF ) * a.size() ) != 0 )
			fail( name + ": device-only and host-current inputs give different bits" );
		const std::vector<MF> & d = std::as_const( dev ).get_buffer();
		if( d.size() != saved.size() || std::memcmp( d.data(), saved.data(), sizeof( MF ) * d.size() ) != 0 ) fail( name + ": the device-only copy changed" );
		}
	};

// ---- the cases every small input runs --------------------------------------------------------------------------------------------------
void run_small( Runner & R, const std::string & tag, const PV & in, const PV & B )
	{
	R.begin( in );
	auto N = [&]( const char * n ){ return std::string( n ) + "." + tag; };

	R.put_audio( N( "convert_to_audio.input" ), in );

	R.put( N( "modify_time.monotone" ), in.modify_time( mt_mono ) );
	R.put( N( "modify_time.backwards" ), in.modify_time( mt_back ) );
	R.put( N( "modify_time.lastmax" ), in.modify_time( mt_lastmax, Interpolator::smoothstep() ) );
	R.put( N( "modify_time.const" ), in.modify_time( c_mt ) );

		{
		const PV s2 = in.stretch( 2.0f );
		R.put_audio( N( "convert_to_audio.stretch.const2" ), s2 );
		R.put( N( "stretch.const2" ), s2 );
		const PV sc = in.stretch( st_tf );
		R.put_audio( N( "convert_to_audio.stretch.callable" ), sc );
		R.put( N( "stretch.callable" ), sc );
		}
	R.put( N( "stretch.const_half" ), in.stretch( 0.5f, Interpolator::nearest() ) );
	R.put( N( "stretch.callable_smootherstep" ), in.stretch( st_tf, Interpolator::smootherstep() ) );

	R.put_both( N( "modify_frequency.callable" ), in, []( const PV & p ){ return p.modify_frequency( mfq ); } );
	R.put( N( "modify_frequency.const" ), in.modify_frequency( c_mfq, Interpolator::smoothstep() ) );
	R.put( N( "repitch.callable" ), in.repitch( rp ) );
	R.put( N( "repitch.const" ), in.repitch( c_rp, Interpolator::smoothstep() ) );
	R.put_both( N( "modify.callable" ), in, []( const PV & p ){ return p.modify( md ); } );
	R.put( N( "modify.const" ), in.modify( c_md ) );
	R.put( N( "modify.ten_minutes" ), in.modify( md_long ) );

	for( const bool align : { false, true } )
		{
		const std::string t = align ? "aligned" : "plain";
		R.put_both( N( ( "shape." + t ).c_str() ), in, [align]( const PV & p ){ return p.shape( shaper, align ); }, align ? "" : N( "convert_to_audio.shape.plain" ) );
		const PV sa = in.shape_affine( 0.5f, 0.001f, 1.02f, 10.0f, align );
		if( !align ) R.put_audio( N( "convert_to_audio.shape_affine.plain" ), sa );
		R.put( N( ( "shape_affine." + t ).c_str() ), sa );
		}

	R.put( N( "replace_amplitudes.callable" ), in.replace_amplitudes( B, amt ) );
	R.put( N( "replace_amplitudes.const" ), in.replace_amplitudes( B, c_amt ) );
	R.put( N( "subtract_amplitudes.callable" ), in.subtract_amplitudes( B, amt ) );
	R.put( N( "subtract_amplitudes.const" ), in.subtract_amplitudes( B, c_amt ) );
	R.put( N( "retain_n_loudest_partials.callable" ), in.retain_n_loudest_partials( nl ) );
	R.put( N( "retain_n_loudest_partials.const" ), in.retain_n_loudest_partials( c_nl ) );
	R.put( N( "remove_n_loudest_partials.callable" ), in.remove_n_loudest_partials( nl ) );
	R.put( N( "remove_n_loudest_partials.const" ), in.remove_n_loudest_partials( c_nl ) );

	R.put( N( "resonate.zero_const" ), in.resonate( 0.0f, c_dc ) );
	R.put( N( "resonate.negative_const" ), in.resonate( -0.3f, c_dc ) );
	R.put( N( "resonate.fractional_const" ), in.resonate( 0.0301f, c_dc ) );
	R.put( N( "resonate.fractional_callable" ), in.resonate( 0.0301f, dc ) );
	R.put( N( "resonate.zero_callable" ), in.resonate( 0.0f, dc ) );

	R.put( N( "desample.callable_linear" ), in.desample( ds, Interpolator::linear() ) );
	R.put( N( "desample.callable_smoothstep" ), in.desample( ds, Interpolator::smoothstep() ) );
	R.put( N( "desample.const" ), in.desample( c_ds ) );

	R.put( N( "time_extrapolate.default_end" ), in.time_extrapolate( 0.02f, -1, 0.03f ) );
	R.put( N( "time_extrapolate.outside" ), in.time_extrapolate( -1.0f, 5.0f, 0.0171f ) );
	R.put( N( "time_extrapolate.inner" ), in.time_extrapolate( 0.0131f, 0.0577f, 0.05f, Interpolator::smoothstep() ) );
	R.put( N( "time_extrapolate.refuse_order" ), in.time_extrapolate( 0.05f, 0.01f, 0.03f ) );
	R.put( N( "time_extrapolate.refuse_length" ), in.time_extrapolate( 0.01f, 0.05f, 0.0f ) );

	R.put( N( "get_frame.negative" ), in.get_frame( -0.5f ) );
	R.put( N( "get_frame.beyond" ), in.get_frame( 10.0f ) );
	R.put( N( "get_frame.on" ), in.get_frame( in.frame_to_time( 20.0f ) ) );
	R.put( N( "get_frame.between" ), in.get_frame( 0.0333f ) );

	R.put( N( "select.shorter" ), in.select( 0.04f, sel ) );
	R.put( N( "select.longer" ), in.select( 0.15f, sel ) );
	R.put( N( "select.const" ), in.select( 0.0507f, c_sel ) );
	R.put( N( "select.refuse" ), in.select( 0.0f, sel ) );

	R.put( N( "freeze.mixed" ), in.freeze( { 0.05f, 0.02f, 0.02f, 10.0f }, { 0.01f, 0.004f, 0.008f, 0.006f } ) );
	R.put( N( "freeze.none" ), in.freeze( {}, {} ) );

	R.put( N( "stretch_spline.callable" ), in.stretch_spline( sp ) );
	R.put( N( "stretch_spline.const" ), in.stretch_spline( c_sp ) );

	R.put( N( "smear_time.const_const_default" ), in.smear_time( c_sm, c_gr ) );
	R.put( N( "smear_time.callable_callable_rational" ), in.smear_time( sm, gr, dist_rat ) );
	R.put( N( "smear_time.const_callable_box" ), in.smear_time( c_sm, gr, 1.0f ) );
	R.put( N( "smear_time.callable_const_default" ), in.smear_time( sm, c_gr ) );

	R.put( N( "add_octaves.callable" ), in.add_octaves( hs ) );
	R.put( N( "add_octaves.const" ), in.add_octaves( c_hs ) );
	R.put( N( "add_harmonics.callable" ), in.add_harmonics( hs ) );
	R.put( N( "add_harmonics.const" ), in.add_harmonics( c_hs ) );

	R.put( N( "cut_frames.inner" ), in.cut_frames( 10, 30 ) );
	R.put( N( "cut_frames.clamped" ), in.cut_frames( -5, 1000 ) );
	R.put( N( "cut_frames.empty" ), in.cut_frames( 30, 30 ) );
	R.put( N( "cut_frames.reversed" ), in.cut_frames( 40, 20 ) );

		{
		const std::vector<PV> pieces = in.split_at_times( { 0.05f, -0.01f, 0.02f, 0.02f, 5.0f, 0.001f } );
		for( size_t i = 0; i < pieces.size(); ++i ) R.put( N( "split_at_times.mixed" ) + "#" + std::to_string( i ), pieces[i] );
		R.put( N( "split_at_times.mixed" ) + "#join", PV::join( pieces ) );
		std::printf( "case %s: %d pieces\n", N( "split_at_times.mixed" ).c_str(), int( pieces.size() ) );
		}
		{
		const PV a = in.cut_frames( 10, 30 ), b = in.cut_frames( 0, 7 );
		R.put( N( "join.mixed" ), PV::join( std::vector<const PV *>{ &a, &B, &in, &b } ) );
		}
	}

void run_big( Runner & R, const PV & in )
	{
	R.begin( in );
	R.put( "stretch.callable_big.BIG", in.stretch( st_big ) );
	R.put( "modify_time.callable_big.BIG", in.modify_time( mt_big ) );
	R.put_both( "shape.plain.BIG", in, []( const PV & p ){ return p.shape( shaper, false ); } );
	R.put_both( "modify_frequency.callable_big.BIG", in, []( const PV & p ){ return p.modify_frequency( mfq_big ); } );
	}

// ---- --sample-only ---------------------------------------------------------------------------------------------------------------------
template<typename T> constexpr int32_t kind_of() { return std::is_same_v<T, float> ? 0 : std::is_same_v<T, int32_t> ? 1 : 2; }

template<typename T>
void dump( const std::string & dir, const std::string & name, const T * data, size_t count )
	{
	const int32_t head[2] = { kind_of<T>(), int32_t( count ) };
	write_file( dir + "/" + name + ".bin", head, sizeof( head ), data, sizeof( T ) * count );
	std::printf( "dump %s: %d\n", name.c_str(), int( count ) );
	}

template<typename Fn>
void dump_grid( const std::string & dir, const std::string & name, const PV & pv, const Fn & fn, Frame frames = -1 )
	{
	using O = decltype( fn( TF{} ) );
	const Function<TF, O> f( fn );
	const auto s = frames < 0 ? pv.sample_function_over_domain( f )
		: f.sample( 0, float( frames ), 1.0f / pv.get_analysis_rate(), 0, float( pv.get_num_bins() ), pv.bin_to_frequency( 1 ) );   // resonate's and select's call
	if( s.is_constant() ) { fail( name + ": constant" ); return; }
	if constexpr( std::is_same_v<O, TF> ) dump( dir, name, reinterpret_cast<const float*>( s.get_vector().data() ), 2 * s.size() );
	else dump( dir, name, s.get_vector().data(), s.size() );
	}

// stretch_spline's per-frame loop (PV.cpp of this project, from PVModify.cpp:391-394), restated
std::vector<uint32_t> spline_steps( const PV & pv, const Function<Second, float> & interpolation )
	{
	std::vector<uint32_t> steps( size_t( pv.get_num_frames() - 1 ) );
	const float seconds_per_frame = pv.frame_to_time( 1 );
	for( Frame frame = 0; frame + 1 < pv.get_num_frames(); ++frame )
		{
		const float v = interpolation( frame * seconds_per_frame );
		const uint32_t u = !( v >= 1.0f ) ? 0u : ( v >= 4294967296.0f ? 0xFFFFFFFFu : uint32_t( v ) );
		steps[size_t( frame )] = std::max( u, 1u );
		}
	return steps;
	}

// harmonic_scale's per-frame loop (from PV.cpp:371-379), restated
std::vector<float> harmonic_series( const PV & pv, const Function<std::pair<Second, Harmonic>, float> & series, Harmonic H )
	{
	std::vector<float> sampled( size_t( H ) * pv.get_num_frames() );
	for( Frame frame = 0; frame < pv.get_num_frames(); ++frame )
		{
		const Second t = pv.frame_to_time( fFrame( frame ) );
		for( Harmonic h = 0; h < H; ++h ) sampled[size_t( h ) + size_t( frame ) * H] = series( std::pair<Second, Harmonic>( t, h ) );
		}
	return sampled;
	}

// smear_time's distribution call (from PVModify.cpp:555-560): dist_samples_2 from the largest smear size, then Function::sample
void dump_distribution( const std::string & dir, const std::string & name, const PV & pv, float largest_smear, const Function<Second, float> & distribution )
	{
	const int32_t expansion = std::max( int32_t( pv.time_to_frame( std::max( largest_smear, 0.0f ) ) ), 0 ), dist_samples_2 = expansion * 2;
	const auto sampled = distribution.sample( -dist_samples_2, dist_samples_2, 1.0f / dist_samples_2 );
	if( sampled.is_constant() ) { fail( name + ": constant" ); return; }
	dump( dir, name, sampled.get_vector().data(), sampled.get_vector().size() );
	}

void sample_only( const std::string & dir )
	{
	for( const std::string tag : { "A", "X" } )
		{
		const PV pv = PV::create_from_format( format_of( tag ) );
		auto N = [&]( const char * n ){ return std::string( n ) + "." + tag; };
		dump_grid( dir, N( "grid.mt_mono" ), pv, mt_mono );
		dump_grid( dir, N( "grid.mt_back" ), pv, mt_back );
		dump_grid( dir, N( "grid.mt_lastmax" ), pv, mt_lastmax );
		dump_grid( dir, N( "grid.st_tf" ), pv, st_tf );
		dump_grid( dir, N( "grid.mfq" ), pv, mfq );
		dump_grid( dir, N( "grid.rp" ), pv, rp );
		dump_grid( dir, N( "grid.amt" ), pv, amt );
		dump_grid( dir, N( "grid.ds" ), pv, ds );
		dump_grid( dir, N( "grid.sm" ), pv, sm );
		dump_grid( dir, N( "grid.gr" ), pv, gr );
		dump_grid( dir, N( "grid.md" ), pv, md );
		dump_grid( dir, N( "grid.md_long" ), pv, md_long );
		dump_grid( dir, N( "outgrid.dc" ), pv, dc, 2 * pv.get_num_frames() );
		dump_grid( dir, N( "outgrid.sel" ), pv, sel, 2 * pv.get_num_frames() );
			{
			const auto sampled = Function<Second, Bin>( nl ).sample( 0, pv.get_num_frames(), pv.frame_to_time( 1 ) );   // n_loudest's call
			dump( dir, N( "bins.nl" ), sampled.get_vector().data(), sampled.get_vector().size() );
			}
		const auto steps = spline_steps( pv, sp ), steps_c = spline_steps( pv, c_sp );
		dump( dir, N( "steps.sp" ), steps.data(), steps.size() );
		dump( dir, N( "steps.const" ), steps_c.data(), steps_c.size() );
		const Harmonic octaves = Harmonic( std::ceil( std::log2( pv.get_height() ) ) );
		const auto so = harmonic_series( pv, hs, octaves ), sh = harmonic_series( pv, hs, pv.get_num_bins() );
		dump( dir, N( "series.hs.octaves" ), so.data(), so.size() );
		dump( dir, N( "series.hs.harmonics" ), sh.data(), sh.size() );
		const auto smear_grid = pv.sample_function_over_domain( Function<TF, Second>( sm ) );
		const float largest = *std::max_element( smear_grid.get_vector().begin(), smear_grid.get_vector().end() );
		const auto raised_cosine = []( Second t ){ return float( 0.5f * ( 1.0f + std::cos( 3.14159265358979323846 * t ) ) ); };   // smear_time's default argument
		dump_distribution( dir, N( "dist.dist_rat.const" ), pv, c_sm, dist_rat );
		dump_distribution( dir, N( "dist.dist_rat.sm" ), pv, largest, dist_rat );
		dump_distribution( dir, N( "dist.default.const" ), pv, c_sm, raised_cosine );
		dump_distribution( dir, N( "dist.default.sm" ), pv, largest, raised_cosine );
		}
	const PV big = PV::create_from_format( format_of( "BIG" ) );
	dump_grid( dir, "grid.mt_big.BIG", big, mt_big );
	dump_grid( dir, "grid.st_big.BIG", big, st_big );
	dump_grid( dir, "grid.mfq_big.BIG", big, mfq_big );
	}

}

int main( int argc, char ** argv )
	{
	const std::string mode = argc > 1 ? argv[1] : "";
	if( mode == "--sample-only" && argc == 3 ) sample_only( argv[2] );
	else if( mode == "--run" && argc == 4 )
		{
		Runner R;
		R.out_dir = argv[3];
		const PV A = read_pv( argv[2], "A" ), X = read_pv( argv[2], "X" ), B = read_pv( argv[2], "B" );
		if( failures == 0 )
			{
			run_small( R, "A", A, B );
			run_small( R, "X", X, B );
			const PV big = read_pv( argv[2], "BIG" );
			if( failures == 0 ) run_big( R, big );
			}
		}
	else { std::printf( "usage: pv_methods_test --run IN_DIR OUT_DIR | --sample-only OUT_DIR\n" ); return 2; }
	std::printf( "\n%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures );
	return failures ? 1 : 0;
	}
