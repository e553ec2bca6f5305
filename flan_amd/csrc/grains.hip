// grains.hip -- the sink of the reference's composition layer, Audio::mix (Audio/AudioCombination.cpp:102-170), with the grains of
// Audio::granulate / psola (Audio/AudioSynthesis.cpp:572-638) cut, faded and windowed in flight.  DESIGN.md section 4.22.
//
// An event is one term of mix: n frames of a source from frame s, added to the output from frame o with a gain.  The reference makes
// every grain an Audio (cut_frames, AudioTemporal.cpp:207-234; fade_frames_in_place with Interpolator::sqrt(), AudioVolume.cpp:102-135;
// psola's Hann window, AudioSynthesis.cpp:626) and adds them one after another (:155-167).  Here an output sample is a gather: the
// ordered fp32 sum, from +0.0f, of the events that cover it, each term read from its source and shaped on the way:
//   v = src[c][s + i], i = g - o
//   i < sf:       v *= sqrtf( float( i ) / sf )                  the start fade
//   i >= n - ef:  v *= sqrtf( float( n - 1 - i ) / ef )          the end fade (sf + ef <= n: the ramps never share a frame)
//   Hann:         v *= float( 0.5 * ( 1.0 - cos( double( 2.0f * pi * ( ( i * ( 1.0f / sr ) ) / ( n / sr ) ) ) ) ) )      WindowFunctions.cpp:10-13
//   v * gain, rounded; then the addition, rounded (-ffp-contract=off: never one fused operation)
// k_grains_mix: a block owns GR_TILE consecutive output frames of one channel, a thread GR_FRAMES of them GR_THREADS apart (so a
// wavefront reads consecutive source frames).  The tile's candidate events -- the index range [first, last] of the plan -- come through
// LDS GR_BATCH at a time: a thread stages one event (its range against the tile's, its pointers for this channel), then every thread
// walks the batch in index order.  An event that misses the tile or the channel is staged with n = 0 and costs the walk one uniform
// branch.  No atomics, no partial sums: the order of additions is the index order whatever the events' start frames.
// The plan is host work (grains_plan): per tile the first and the last event index that touch it, O( events + overlaps ).
// The event generator (integrate_event_rate, AudioSynthesis.cpp:310-374) and the cut validation are host arithmetic as well.
#include "flanhip_internal.h"

#include <climits>
#include <cstring>

namespace flanhip {

namespace {

constexpr int GR_THREADS = 256;
constexpr int GR_FRAMES = 4;                                   // output frames per thread
constexpr int GR_TILE = GR_THREADS * GR_FRAMES;                // 1024 output frames per block
constexpr int GR_BATCH = GR_THREADS;                           // events staged per round: one per thread, 40 bytes each, 10 KiB of LDS

struct GrStaged                                                // an event as the walk reads it: every thread the same address, a broadcast
	{
	const float * src;                                         // the source at ( channel, s )
	const float * gains;                                       // per-frame gains at local frame 0, or null
	int rel;                                                   // o - the tile's first frame; in ( -n, GR_TILE ) when n > 0
	int n;                                                     // 0: not on this tile or channel
	int sf, ef;
	int hann;
	float gain;
	};

__global__ __launch_bounds__( GR_THREADS ) void k_grains_mix( const flanhip_grain_event * __restrict__ events, const int * __restrict__ tile_first,
	const int * __restrict__ tile_last, const float * __restrict__ gains, const float * __restrict__ sources, int64_t num_tiles, int64_t out_frames,
	float step, float sample_rate, float * __restrict__ out )
	{
	__shared__ GrStaged staged[GR_BATCH];
	const int tid = threadIdx.x;
	const int64_t tile = int64_t( blockIdx.x ) % num_tiles;
	const int channel = int( int64_t( blockIdx.x ) / num_tiles );
	const int64_t tile0 = tile * GR_TILE;
	const int first = tile_first[tile], last = tile_last[tile];

	float acc[GR_FRAMES];
	#pragma unroll
	for( int k = 0; k < GR_FRAMES; ++k ) acc[k] = 0.0f;                       // out.clear_buffer() (:152)

	for( int base = first; base <= last; base += GR_BATCH )
		{
		const int count = last - base + 1 < GR_BATCH ? last - base + 1 : GR_BATCH;
		if( tid < count )
			{
			const flanhip_grain_event e = events[base + tid];
			const int64_t rel = e.o - tile0;
			const bool live = e.n > 0 && channel < e.channels && rel < GR_TILE && rel + e.n > 0;
			GrStaged g;
			const float * src = sources ? sources + e.src : reinterpret_cast<const float*>( uintptr_t( e.src ) );
			g.src = src + int64_t( channel ) * e.ch_stride + e.s;
			g.gains = e.gain_offset >= 0 ? gains + e.gain_offset : nullptr;
			g.rel = live ? int( rel ) : 0;
			g.n = live ? e.n : 0;
			g.sf = e.sf; g.ef = e.ef;
			g.hann = e.flags & FLANHIP_GRAIN_HANN;
			g.gain = e.gain;
			staged[tid] = g;
			}
		__syncthreads();
		for( int j = 0; j < count; ++j )
			{
			const int n = staged[j].n;
			if( n == 0 ) continue;
			const GrStaged g = staged[j];
			#pragma unroll
			for( int k = 0; k < GR_FRAMES; ++k )
				{
				const int i = tid + k * GR_THREADS - g.rel;
				if( unsigned( i ) < unsigned( n ) )
					{
					float v = g.src[i];
					if( i < g.sf ) v *= sqrtf( float( i ) / float( g.sf ) );
					if( i >= n - g.ef ) v *= sqrtf( float( n - 1 - i ) / float( g.ef ) );
					if( g.hann )
						{
						const float x = ( float( i ) * step ) / ( float( n ) / sample_rate );
						const float a = 6.2831855f * x;                               // 2.0f * pi, pi = acos( -1.0f )
						v *= float( 0.5 * ( 1.0 - cos( double( a ) ) ) );            // the reference's unqualified cos is the double one
						}
					const float term = v * ( g.gains ? g.gains[i] : g.gain );
					acc[k] = acc[k] + term;
					}
				}
			}
		__syncthreads();
		}

	float * row = out + int64_t( channel ) * out_frames + tile0;
	#pragma unroll
	for( int k = 0; k < GR_FRAMES; ++k )
		{
		const int f = tid + k * GR_THREADS;
		if( tile0 + f < out_frames ) row[f] = acc[k];
		}
	}

// ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
int64_t grains_num_tiles( int64_t out_frames ) { return ( out_frames + GR_TILE - 1 ) / GR_TILE; }

// AudioCombination.cpp:146-150: the maximum of start + frames over ALL events, the empty ones too, from 0
int64_t grains_out_frames( const flanhip_grain_event * events, int64_t count )
	{
	int64_t frames = 0;
	for( int64_t i = 0; i < count; ++i ) frames = std::max( frames, events[i].o + int64_t( std::max( events[i].n, 0 ) ) );
	return frames;
	}

// per tile of out_frames the first and the last event index that touch it; ( 0, -1 ): none
void grains_plan( const flanhip_grain_event * events, int64_t count, int64_t out_frames, int32_t * first, int32_t * last )
	{
	const int64_t tiles = grains_num_tiles( out_frames );
	for( int64_t t = 0; t < tiles; ++t ) { first[t] = INT_MAX; last[t] = -1; }
	for( int64_t i = 0; i < count; ++i )
		{
		const flanhip_grain_event & e = events[i];
		if( e.n <= 0 || e.channels <= 0 ) continue;
		const int64_t lo = std::max<int64_t>( e.o, 0 ), hi = std::min<int64_t>( e.o + e.n, out_frames );      // [lo, hi)
		if( lo >= hi ) continue;
		for( int64_t t = lo / GR_TILE; t <= ( hi - 1 ) / GR_TILE; ++t )
			{
			if( first[t] == INT_MAX ) first[t] = int32_t( i );
			last[t] = int32_t( i );
			}
		}
	for( int64_t t = 0; t < tiles; ++t ) if( first[t] == INT_MAX ) first[t] = 0;
	}

// what the kernel would read through: every live event inside its source, its gains inside the pool
int grains_check_events( const flanhip_grain_event * events, int64_t count, bool have_gains, int64_t gain_floats, bool have_base, int64_t sources_floats )
	{
	FLANHIP_REQUIRE( count >= 0 && count < INT_MAX, FLANHIP_ERR_INVALID_ARG, "event count out of range" );
	FLANHIP_REQUIRE( events || count == 0, FLANHIP_ERR_INVALID_ARG, "null event table" );
	for( int64_t i = 0; i < count; ++i )
		{
		const flanhip_grain_event & e = events[i];
		FLANHIP_REQUIRE( e.n >= 0 && e.channels >= 0, FLANHIP_ERR_INVALID_ARG, "an event with a negative size" );
		FLANHIP_REQUIRE( ( e.flags & ~FLANHIP_GRAIN_HANN ) == 0, FLANHIP_ERR_INVALID_ARG, "an event with unknown flags" );
		FLANHIP_REQUIRE( e.o > -( int64_t( 1 ) << 60 ) && e.o < ( int64_t( 1 ) << 60 ), FLANHIP_ERR_INVALID_ARG, "an event's output frame out of range" );
		if( e.n == 0 || e.channels == 0 ) continue;
		FLANHIP_REQUIRE( e.s >= 0 && e.src_frames >= 0 && int64_t( e.s ) + e.n <= e.src_frames && e.ch_stride >= 0, FLANHIP_ERR_INVALID_ARG,
			"an event's source range leaves its buffer" );
		if( have_base )
			FLANHIP_REQUIRE( e.src <= uint64_t( sources_floats ) && e.ch_stride <= sources_floats && e.src_frames <= sources_floats
				&& int64_t( e.src ) + int64_t( e.channels - 1 ) * e.ch_stride + e.src_frames <= sources_floats, FLANHIP_ERR_INVALID_ARG,
				"an event's source range leaves its buffer" );
		else
			FLANHIP_REQUIRE( e.src != 0, FLANHIP_ERR_INVALID_ARG, "an event with a null source" );
		FLANHIP_REQUIRE( e.sf >= 0 && e.ef >= 0 && int64_t( e.sf ) + e.ef <= e.n, FLANHIP_ERR_INVALID_ARG, "an event's fades are longer than the event" );
		if( e.gain_offset >= 0 )
			FLANHIP_REQUIRE( have_gains && e.gain_offset <= gain_floats && e.gain_offset + e.n <= gain_floats, FLANHIP_ERR_INVALID_ARG,
				"an event's gains leave the pool" );
		}
	return FLANHIP_OK;
	}

struct GrLayout { size_t events_off, first_off, last_off, total; };
GrLayout grains_layout( int64_t count, int64_t tiles )
	{
	const auto up = []( size_t v ){ return ( v + 255 ) & ~size_t( 255 ); };
	GrLayout l;
	l.events_off = 0;
	l.first_off = up( sizeof( flanhip_grain_event ) * size_t( std::max<int64_t>( count, 1 ) ) );
	l.last_off = l.first_off + up( sizeof( int32_t ) * size_t( std::max<int64_t>( tiles, 1 ) ) );
	l.total = l.last_off + up( sizeof( int32_t ) * size_t( std::max<int64_t>( tiles, 1 ) ) );
	return l;
	}

// the table and the plan into the workspace, one launch
int launch_grains( const flanhip_grain_event * events, int64_t count, const int32_t * first, const int32_t * last, int64_t tiles, const float * d_gains,
	const float * d_sources, int64_t channels, int64_t out_frames, float sample_rate, float * d_out, void * d_ws, hipStream_t s )
	{
	const GrLayout l = grains_layout( count, tiles );
	char * ws = static_cast<char*>( d_ws );
	if( count > 0 ) FLANHIP_CHECK( hipMemcpyAsync( ws + l.events_off, events, sizeof( flanhip_grain_event ) * size_t( count ), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipMemcpyAsync( ws + l.first_off, first, sizeof( int32_t ) * size_t( tiles ), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipMemcpyAsync( ws + l.last_off, last, sizeof( int32_t ) * size_t( tiles ), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipStreamSynchronize( s ) );                                  // the host tables may go once the copies have read them
	return launch_kernel( "launch_grains", k_grains_mix, tiles * channels, GR_THREADS, 0, s, ws_at<const flanhip_grain_event>( d_ws, l.events_off ),
		ws_at<const int>( d_ws, l.first_off ), ws_at<const int>( d_ws, l.last_off ), d_gains, d_sources, tiles, out_frames, 1.0f / sample_rate, sample_rate, d_out );
	}

// a time as a Frame (time_to_frame truncated, AudioBuffer.cpp:406-409): false for what no int holds (NaN, infinities, beyond the range)
bool time_to_frame_checked( float t, float sample_rate, int32_t * frame )
	{
	const float f = t * sample_rate;
	if( !( f > -2147483648.0f && f < 2147483648.0f ) ) return false;
	*frame = int32_t( f );
	return true;
	}

// AudioTemporal.cpp:207-234 with the validation of AudioVolume.cpp:111-118: s, n, sf, ef of one event
void cut_frames_event( int64_t num_frames, int32_t start, int32_t end, int32_t start_fade, int32_t end_fade, flanhip_grain_event * e )
	{
	e->s = 0; e->n = 0; e->sf = 0; e->ef = 0;
	if( end <= start ) return;                                                   // :217, before the clamp
	const int32_t top = int32_t( std::min<int64_t>( num_frames - 1, INT_MAX ) );
	start = std::clamp( start, 0, top );                                         // :218-219
	end = std::clamp( end, 0, top );
	const int32_t n = end - start;
	if( n <= 0 ) return;
	int64_t sf = std::max( 0, start_fade ), ef = std::max( 0, end_fade );       // AudioVolume.cpp:111-112
	if( sf + ef > n )
		{
		const float scale = float( n ) / float( sf + ef );                       // :115-117
		sf = int64_t( std::floor( float( sf ) * scale ) );
		ef = int64_t( std::floor( float( ef ) * scale ) );
		}
	e->s = start; e->n = n; e->sf = int32_t( sf ); e->ef = int32_t( ef );
	}

// a uniform 64-bit stream (splitmix64) and normal deviates from it by Box and Muller in double
struct GrRng
	{
	uint64_t state;
	uint64_t next() { uint64_t z = ( state += 0x9E3779B97F4A7C15ull ); z = ( z ^ ( z >> 30 ) ) * 0xBF58476D1CE4E5B9ull; z = ( z ^ ( z >> 27 ) ) * 0x94D049BB133111EBull; return z ^ ( z >> 31 ); }
	double uniform() { return ( double( next() >> 11 ) + 0.5 ) * ( 1.0 / 9007199254740992.0 ); }      // in ( 0, 1 )
	double normal() { const double u = uniform(), v = uniform(); return std::sqrt( -2.0 * std::log( u ) ) * std::cos( 6.283185307179586 * v ); }
	};

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int64_t flanhip_grains_tile_frames( void ) { return GR_TILE; }
int64_t flanhip_grains_batch_events( void ) { return GR_BATCH; }

int flanhip_grains_events( int64_t length_frames, float sample_rate, const float * rate, float rate_scalar, const float * scatter, float scatter_scalar,
	uint64_t seed, int64_t * out_frames, int64_t capacity, int64_t * out_count )
	{
	FLANHIP_REQUIRE( out_count, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( length_frames > 0 && length_frames < INT_MAX, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sample_rate > 0, FLANHIP_ERR_INVALID_ARG, "sample_rate <= 0" );
	FLANHIP_REQUIRE( capacity >= 0 && ( out_frames || capacity == 0 ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	const auto rate_at = [&]( int64_t f ){ return std::max( 0.0f, rate ? rate[f] : rate_scalar ); };              // :320
	const auto scatter_at = [&]( int64_t f ){ return std::max( 0.0f, scatter ? scatter[f] : scatter_scalar ); };  // :323
	std::vector<int64_t> frames;
	float accumulator = 1.0f;                                                    // :328-338
	for( int64_t frame = 0; frame < length_frames; ++frame )
		{
		accumulator += rate_at( frame ) / sample_rate;
		if( accumulator >= 1.0f )
			{
			frames.push_back( frame );
			accumulator -= std::floor( accumulator );
			}
		}
	GrRng rng{ seed };
	bool scattered = false;
	for( int64_t & frame : frames )                                              // :343-358
		{
		const float scatter_t = scatter_at( frame ), rate_t = rate_at( frame );
		if( scatter_t == 0 || rate_t == 0 ) continue;
		const float std_in_seconds = scatter_t / rate_t;
		const float std_in_frames = std_in_seconds * sample_rate;
		const float moved = float( double( float( frame ) ) + double( std_in_frames ) * rng.normal() );
		scattered = true;
		if( moved >= 0.0f && moved < float( length_frames ) && int64_t( moved ) < length_frames ) frame = int64_t( moved );
		else frame = INT64_MAX;
		}
	if( scattered )
		{
		std::sort( frames.begin(), frames.end() );                               // :361-366
		frames.erase( std::lower_bound( frames.begin(), frames.end(), INT64_MAX ), frames.end() );
		}
	*out_count = int64_t( frames.size() );
	if( capacity == 0 ) return FLANHIP_OK;                                       // the count alone
	FLANHIP_REQUIRE( capacity >= int64_t( frames.size() ), FLANHIP_ERR_INVALID_ARG, "the event buffer is too small" );
	std::copy( frames.begin(), frames.end(), out_frames );
	return FLANHIP_OK;
	}

int flanhip_grains_cut_frames( int64_t num_frames, int64_t count, const int32_t * start, const int32_t * end, const int32_t * start_fade,
	const int32_t * end_fade, flanhip_grain_event * events )
	{
	FLANHIP_REQUIRE( num_frames > 0 && count >= 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( count == 0 || ( start && end && start_fade && end_fade && events ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	for( int64_t i = 0; i < count; ++i ) cut_frames_event( num_frames, start[i], end[i], start_fade[i], end_fade[i], events + i );
	return FLANHIP_OK;
	}

int flanhip_grains_cut( int64_t num_frames, float sample_rate, int64_t count, const float * start_time, const float * end_time, const float * start_fade,
	const float * end_fade, flanhip_grain_event * events )
	{
	FLANHIP_REQUIRE( num_frames > 0 && count >= 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sample_rate > 0, FLANHIP_ERR_INVALID_ARG, "sample_rate <= 0" );
	FLANHIP_REQUIRE( count == 0 || ( start_time && end_time && start_fade && end_fade && events ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	for( int64_t i = 0; i < count; ++i )
		{
		int32_t s, e, sf, ef;
		if( time_to_frame_checked( start_time[i], sample_rate, &s ) && time_to_frame_checked( end_time[i], sample_rate, &e )
			&& time_to_frame_checked( start_fade[i], sample_rate, &sf ) && time_to_frame_checked( end_fade[i], sample_rate, &ef ) )
			cut_frames_event( num_frames, s, e, sf, ef, events + i );
		else { events[i].s = 0; events[i].n = 0; events[i].sf = 0; events[i].ef = 0; }      // no Frame holds it: an empty event
		}
	return FLANHIP_OK;
	}

int flanhip_grains_plan( const flanhip_grain_event * events, int64_t count, int64_t * out_frames, int32_t * tile_first, int32_t * tile_last, int64_t num_tiles )
	{
	FLANHIP_REQUIRE( out_frames, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count >= 0 && count < INT_MAX, FLANHIP_ERR_INVALID_ARG, "event count out of range" );
	FLANHIP_REQUIRE( events || count == 0, FLANHIP_ERR_INVALID_ARG, "null event table" );
	for( int64_t i = 0; i < count; ++i )
		FLANHIP_REQUIRE( events[i].n >= 0 && events[i].o > -( int64_t( 1 ) << 60 ) && events[i].o < ( int64_t( 1 ) << 60 ), FLANHIP_ERR_INVALID_ARG,
			"an event's output range out of range" );
	const int64_t frames = *out_frames > 0 ? *out_frames : grains_out_frames( events, count );      // the caller's length, or the reference's
	*out_frames = frames;
	if( !tile_first && !tile_last ) return FLANHIP_OK;                           // the length alone
	FLANHIP_REQUIRE( tile_first && tile_last, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_tiles == grains_num_tiles( frames ), FLANHIP_ERR_INVALID_ARG, "num_tiles is not the output's tile count" );
	grains_plan( events, count, frames, tile_first, tile_last );
	return FLANHIP_OK;
	}

size_t flanhip_grains_workspace_bytes( int64_t count, int64_t out_frames )
	{
	if( count < 0 || count >= INT_MAX || out_frames <= 0 ) return 0;
	return grains_layout( count, grains_num_tiles( out_frames ) ).total;
	}

static int grains_check_call( const flanhip_grain_event * events, int64_t count, const int32_t * tile_first, const int32_t * tile_last, int64_t num_tiles,
	const float * gains, int64_t gain_floats, const float * sources, int64_t sources_floats, int64_t num_channels, int64_t out_frames, float sample_rate )
	{
	FLANHIP_REQUIRE( num_channels > 0 && out_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sample_rate > 0, FLANHIP_ERR_INVALID_ARG, "sample_rate <= 0" );
	FLANHIP_REQUIRE( gain_floats >= 0 && sources_floats >= 0, FLANHIP_ERR_INVALID_ARG, "negative size" );
	if( int rc = grains_check_events( events, count, gains != nullptr, gain_floats, sources != nullptr, sources_floats ) ) return rc;
	if( tile_first || tile_last || num_tiles )
		{
		FLANHIP_REQUIRE( tile_first && tile_last, FLANHIP_ERR_INVALID_ARG, "null plan" );
		FLANHIP_REQUIRE( num_tiles == grains_num_tiles( out_frames ), FLANHIP_ERR_INVALID_ARG, "num_tiles is not the output's tile count" );
		for( int64_t t = 0; t < num_tiles; ++t )
			FLANHIP_REQUIRE( tile_first[t] >= 0 && tile_last[t] < count && tile_last[t] >= -1, FLANHIP_ERR_INVALID_ARG, "the plan names events the table does not hold" );
		}
	return FLANHIP_OK;
	}

int flanhip_grains_mix_dev( const flanhip_grain_event * events, int64_t count, const int32_t * tile_first, const int32_t * tile_last, int64_t num_tiles,
	const float * d_gains, int64_t gain_floats, const float * d_sources, int64_t sources_floats, int64_t num_channels, int64_t out_frames,
	float sample_rate, float * d_out, void * d_workspace, void * stream )
	{
	FLANHIP_REQUIRE( d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	FLANHIP_REQUIRE( tile_first && tile_last, FLANHIP_ERR_INVALID_ARG, "null plan" );
	if( int rc = grains_check_call( events, count, tile_first, tile_last, num_tiles, d_gains, gain_floats, d_sources, sources_floats, num_channels, out_frames, sample_rate ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_grains( events, count, tile_first, tile_last, num_tiles, d_gains, d_sources, num_channels, out_frames, sample_rate, d_out, d_workspace,
		(hipStream_t) stream );
	}

int flanhip_grains_mix( const flanhip_grain_event * events, int64_t count, const float * gains, int64_t gain_floats, const float * sources, int64_t sources_floats,
	int64_t num_channels, int64_t out_frames, float sample_rate, float * out, volatile int * cancel )
	{
	FLANHIP_REQUIRE( out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( sources || count == 0, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	if( int rc = grains_check_call( events, count, nullptr, nullptr, 0, gains, gain_floats, sources, sources_floats, num_channels, out_frames, sample_rate ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const int64_t tiles = grains_num_tiles( out_frames );
	std::vector<int32_t> first( static_cast<size_t>( tiles ) ), last( static_cast<size_t>( tiles ) );
	grains_plan( events, count, out_frames, first.data(), last.data() );
	HostCall call( cancel );
	const float * d_sources = nullptr, * d_gains = nullptr;
	float * d_out = nullptr;
	void * d_ws = nullptr;
	if( int rc = call.in( sources, sizeof( float ) * size_t( sources_floats ), &d_sources ) ) return rc;
	if( gains ) if( int rc = call.in( gains, sizeof( float ) * size_t( gain_floats ), &d_gains ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( num_channels ) * size_t( out_frames ), &d_out ) ) return rc;
	if( int rc = call.scratch( grains_layout( count, tiles ).total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_grains( events, count, first.data(), last.data(), tiles, d_gains, d_sources, num_channels, out_frames, sample_rate, d_out, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

} // extern "C"
