// volume.hip -- the rest of Audio/AudioVolume.cpp and Audio/AudioInformation.cpp's energies: Audio::ring_modulate (AudioVolume.cpp:15-30), the
// fade family (:69-135), the nonlinearity of Audio::add_moisture (:168-188) between its two resampler chains, the named waveforms
// (Function.cpp:32-39) and Audio::get_total_energy (AudioInformation.cpp:121-129).  DESIGN.md section 4.26.
//
//   k_pointwise<Op>   one launch over the whole [ch][n] block as ONE row of ch * n floats: a lane owns a quad cut at the 16-byte boundaries of
//                     the OUTPUT, whatever n and the rows' alignment are (a quad may span two rows: every element carries its own channel
//                     and frame); one 16-byte store, one 16-byte load where the source is aligned too.  The up to three floats before the
//                     first boundary and the up to three behind the last whole quad go one each to the lanes behind the last quad's: no
//                     lane loops over a ragged end.  Op: out = op( channel, frame, in )
//        RingOp       in * other[c % other_ch][f % other_frames]                                            exact
//        FadeOp       in * start_gain[f] for f < start, then * end_gain[n - 1 - f] for f >= n - end; others copied     exact
//        MoistOp      s + amount * s * waveform( pi2 * frequency * power ), the reference's fp32 products in its order; pow and sin are
//                     evaluated in fp64 on the fp32 arguments and rounded once, so each is the correctly rounded fp32 function
//        WaveOp       waveform( t ) at given phases
//        RectOp       s < 0 ? -s : s, the rectifier of Audio::get_amplitude_envelope (AudioInformation.cpp:331-333)
//   k_energy          per ( channel, block ): the squares, exact in fp64, summed in a fixed order: a lane's own in ascending frames, the
//                     wavefront by halving, the block's wavefronts in order
//   k_energy_close    one block per channel: the block sums in the same fixed order, rounded to fp32 once.  No atomics anywhere.
//
// The oscillator of Audio::synthesize_waveform (Audio/AudioSynthesis.cpp:25-69).  Its phases are the exclusive scan of
// fmod_fixed( a + b, M ), M the oversampled rate (:51-58): a scan of the maps "add c modulo M" over the run_scan.h skeleton, carried in fp64
// -- the phase is an undamped integrator, and an fp32 replay from an fp64 carry would not reproduce the drift of the reference's own,
// unspecified grouping anyway:
//   k_osc_sum         a lane adds the frequencies of its run in fp64 and reduces the sum into [0, M): one map; block_scan; the block's total
//   k_scan_carry      run_scan.h's, over the block totals
//   k_osc_replay      the lane maps again, block_scan, then every frame of the run from the carried fp64 state: phase = float( p / M ), the
//                     named waveform at it where one is asked for, p = ( p + frequency ) modulo M, upward for a negative sum as fmod_fixed
// then() must not see M (run_scan.h finds it by its two arguments), so a map carries M beside c; M == 0 marks the identity, which is also
// k_scan_carry's S{}.
#include "run_scan.h"

#include <climits>
#include <random>

namespace flanhip {

namespace {

constexpr int64_t VOL_MAX_CHANNELS = 1 << 20;
constexpr int VOL_THREADS = 256;
constexpr int ENERGY_QUADS_PER_LANE = 4;
constexpr int64_t ENERGY_BLOCK_QUADS = int64_t( VOL_THREADS ) * ENERGY_QUADS_PER_LANE;      // 4096 frames per block

// ---- the waveforms (Function.cpp:32-39): fmod( t, 1.0f ), which keeps t's sign, then the reference's expression ------------------------
__device__ __forceinline__ float waveform( int kind, float t )
	{
	const float pi2 = 6.2831855f;                                      // defines.h:45: acos( -1.0f ) * 2.0f
	const float t0 = fmodf( t, 1.0f );
	switch( kind )
		{
		case FLANHIP_WAVEFORM_SINE:     return float( sin( double( pi2 * t0 ) ) );     // the fp32 product, then the correctly rounded fp32 sine
		case FLANHIP_WAVEFORM_SQUARE:   return t0 < 0.5f ? -1.0f : 1.0f;
		case FLANHIP_WAVEFORM_SAW:      return -1.0f + 2.0f * t0;
		default:                        return t0 < 0.5f ? -1.0f + 4.0f * t0 : 3.0f - 4.0f * t0;
		}
	}

float waveform_host( int kind, float t )
	{
	const float pi2 = std::acos( -1.0f ) * 2.0f;
	const float t0 = std::fmod( t, 1.0f );
	switch( kind )
		{
		case FLANHIP_WAVEFORM_SINE:     return std::sin( pi2 * t0 );
		case FLANHIP_WAVEFORM_SQUARE:   return t0 < 0.5f ? -1.0f : 1.0f;
		case FLANHIP_WAVEFORM_SAW:      return -1.0f + 2.0f * t0;
		default:                        return t0 < 0.5f ? -1.0f + 4.0f * t0 : 3.0f - 4.0f * t0;
		}
	}

bool valid_waveform( int kind ) { return kind >= FLANHIP_WAVEFORM_SINE && kind <= FLANHIP_WAVEFORM_TRIANGLE; }

// ---- the pointwise operations -----------------------------------------------------------------------------------------------------
struct RingOp
	{
	const float * other; uint32_t other_ch, other_n;
	__device__ __forceinline__ float operator()( int64_t c, int64_t f, float s ) const
		{
		return s * other[int64_t( uint32_t( c ) % other_ch ) * other_n + uint32_t( f ) % other_n];          // :26
		}
	};

struct FadeOp
	{
	const float * start_gain, * end_gain; int64_t n, start, end;
	__device__ __forceinline__ float operator()( int64_t, int64_t f, float s ) const
		{
		if( f < start ) s *= start_gain[f];                              // :123-127
		if( f >= n - end ) s *= end_gain[n - 1 - f];                     // :128-132, after the start's
		return s;
		}
	};

struct MoistOp
	{
	const float * amount, * frequency, * skew; float amount_c, frequency_c, skew_c;
	float sr_over, sr; int64_t n; int kind;
	__device__ __forceinline__ float operator()( int64_t, int64_t F, float s ) const
		{
		const float pi2 = 6.2831855f;
		const float t = float( F ) / sr_over;                            // oversampled.frame_to_time( frame ), :161
		// time_to_frame of the ORIGINAL Audio, truncated (:181-183); clamped into the curves, which the reference's vector is not
		const int64_t i = std::min<int64_t>( std::max<int64_t>( int64_t( t * sr ), 0 ), n - 1 );
		const float a = amount ? amount[i] : amount_c, fr = frequency ? frequency[i] : frequency_c, k = skew ? skew[i] : skew_c;
		const float power = s >= 0 ? float( pow( double( s ), double( k ) ) ) : -float( pow( double( -s ), double( k ) ) );      // :185
		const float w = waveform( kind, pi2 * fr * power );
		return s + a * s * w;                                            // :186 (no contraction: -ffp-contract=off)
		}
	};

struct RectOp                                                          // AudioInformation.cpp:331-333: -0 and a NaN stay as they are
	{
	__device__ __forceinline__ float operator()( int64_t, int64_t, float s ) const { return s < 0 ? s * -1.0f : s; }
	};

struct WaveOp
	{
	int kind;
	__device__ __forceinline__ float operator()( int64_t, int64_t, float t ) const { return waveform( kind, t ); }
	};

// total = ch * n floats; nothing is read or written outside [0, total)
template<typename Op>
__global__ __launch_bounds__( VOL_THREADS ) void k_pointwise( const float * in, float * out, int64_t n, int64_t total, Op op )      // (out may be in)
	{
	const int64_t head = std::min<int64_t>( total, int64_t( ( 4 - ( ( reinterpret_cast<uintptr_t>( out ) >> 2 ) & 3 ) ) & 3 ) );
	const int64_t quads = ( total - head ) / 4;
	const int64_t q = int64_t( blockIdx.x ) * VOL_THREADS + threadIdx.x;
	if( q < quads )
		{
		const int64_t i = head + 4 * q;
		int64_t c = i / n, f = i - c * n;
		const float * s = in + i;
		float4 v;
		if( ( reinterpret_cast<uintptr_t>( s ) & 15 ) == 0 ) v = *reinterpret_cast<const float4*>( s );
		else v = make_float4( s[0], s[1], s[2], s[3] );
		float r[4] = { v.x, v.y, v.z, v.w };
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			{
			r[k] = op( c, f, r[k] );
			if( ++f == n ) { f = 0; ++c; }
			}
		*reinterpret_cast<float4*>( out + i ) = make_float4( r[0], r[1], r[2], r[3] );
		return;
		}
	// the ragged ends, one float per lane: the head's, then those behind the last whole quad
	const int64_t e = q - quads, tail0 = head + 4 * quads;
	const int64_t i = e < head ? e : tail0 + ( e - head );
	if( i >= total ) return;
	const int64_t c = i / n;
	out[i] = op( c, i - c * n, in[i] );
	}

template<typename Op>
int launch_pointwise( const char * who, const float * d_in, float * d_out, int64_t n, int64_t total, const Op & op, hipStream_t s )
	{
	const int64_t lanes = total / 4 + 6;                                // every whole quad and at most 3 + 3 ragged floats
	return launch_kernel( who, k_pointwise<Op>, ( lanes + VOL_THREADS - 1 ) / VOL_THREADS, VOL_THREADS, 0, s, d_in, d_out, n, total, op );
	}

// ---- energy ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum( double mine, double * s_part )
	{
	#pragma unroll
	for( int off = 32; off > 0; off >>= 1 ) mine += __shfl_down( mine, off );
	if( ( threadIdx.x & 63 ) == 0 ) s_part[threadIdx.x >> 6] = mine;
	__syncthreads();
	double sum = s_part[0];
	#pragma unroll
	for( int w = 1; w < VOL_THREADS / 64; ++w ) sum += s_part[w];
	__syncthreads();
	return sum;
	}

// partial: [ch][blocks].  A row's quads are cut at ITS 16-byte boundaries; the up to three frames before the first are the first block's
// lanes 0 ... 2, the up to three behind the last quad the last block's lanes 0 ... 2
__global__ __launch_bounds__( VOL_THREADS ) void k_energy( const float * __restrict__ audio, int64_t n, int64_t blocks, double * __restrict__ partial )
	{
	__shared__ double s_part[VOL_THREADS / 64];
	const int64_t c = int64_t( blockIdx.x ) / blocks, b = int64_t( blockIdx.x ) - c * blocks;
	const float * row = audio + c * n;
	const int64_t head = std::min<int64_t>( n, int64_t( ( 4 - ( ( reinterpret_cast<uintptr_t>( row ) >> 2 ) & 3 ) ) & 3 ) );
	const int64_t quads = ( n - head ) / 4;
	double acc = 0;
	if( b == 0 && threadIdx.x < head ) { const double v = row[threadIdx.x]; acc += v * v; }
	#pragma unroll
	for( int j = 0; j < ENERGY_QUADS_PER_LANE; ++j )
		{
		const int64_t q = b * ENERGY_BLOCK_QUADS + int64_t( j ) * VOL_THREADS + threadIdx.x;
		if( q < quads )
			{
			const float4 v = *reinterpret_cast<const float4*>( row + head + 4 * q );
			acc += double( v.x ) * double( v.x );                             // a product of two fp32 values is exact in fp64
			acc += double( v.y ) * double( v.y );
			acc += double( v.z ) * double( v.z );
			acc += double( v.w ) * double( v.w );
			}
		}
	const int64_t t = head + 4 * quads + threadIdx.x;
	if( b == blocks - 1 && threadIdx.x < 3 && t < n ) { const double v = row[t]; acc += v * v; }
	const double sum = block_sum( acc, s_part );
	if( threadIdx.x == 0 ) partial[c * blocks + b] = sum;
	}

__global__ __launch_bounds__( VOL_THREADS ) void k_energy_close( const double * __restrict__ partial, int64_t blocks, float * __restrict__ energy )
	{
	__shared__ double s_part[VOL_THREADS / 64];
	const double * p = partial + int64_t( blockIdx.x ) * blocks;
	double acc = 0;
	for( int64_t b = threadIdx.x; b < blocks; b += VOL_THREADS ) acc += p[b];
	const double sum = block_sum( acc, s_part );
	if( threadIdx.x == 0 ) energy[blockIdx.x] = float( sum );          // the one rounding to fp32 (an overflow gives inf, as fp32 sums do)
	}

int64_t energy_blocks( int64_t n ) { return ( ( n + 3 ) / 4 + ENERGY_BLOCK_QUADS - 1 ) / ENERGY_BLOCK_QUADS; }

// ---- the oscillator ---------------------------------------------------------------------------------------------------------------
thread_local int t_osc_run = 0;            // flanhip_osc_debug_run: frames per lane forced for the calling thread (0: the library's choice)

struct PhaseMap { double c, m; };          // p -> ( p + c ) modulo m, c in [0, m); m == 0: the identity

struct OscLayout
	{
	int run = 0;
	int64_t blocks = 0;
	size_t tot = 0, carry = 0, total = 0;
	};

bool osc_layout( int64_t n, OscLayout * l )
	{
	if( n <= 0 || n > INT32_MAX ) return false;
	const auto up = []( size_t v ){ return ( v + 255 ) & ~size_t( 255 ); };
	l->run = scan_run( t_osc_run );
	l->blocks = scan_blocks( n, l->run );
	l->tot = 0;
	l->carry = l->tot + up( sizeof( PhaseMap ) * size_t( l->blocks ) );
	l->total = l->carry + up( sizeof( PhaseMap ) * size_t( l->blocks ) );
	return true;
	}

__device__ __forceinline__ void set_identity( PhaseMap & m ) { m = PhaseMap{ 0.0, 0.0 }; }
__device__ __forceinline__ PhaseMap then( const PhaseMap & e, const PhaseMap & l )
	{
	if( l.m == 0.0 ) return e;
	if( e.m == 0.0 ) return l;
	const double s = e.c + l.c;                                        // both in [0, m): below 2 m
	return PhaseMap{ s >= e.m ? s - e.m : s, e.m };
	}
__device__ __forceinline__ PhaseMap apply( const PhaseMap & m, const PhaseMap & state ) { return then( state, m ); }
__device__ __forceinline__ PhaseMap shfl_up( const PhaseMap & m, int off ) { return PhaseMap{ __shfl_up( m.c, off ), __shfl_up( m.m, off ) }; }
// x modulo m into [0, m), upward for a negative x (fmod_fixed, :51-56)
__device__ __forceinline__ double wrap( double x, double m )
	{
	if( x >= 0.0 && x < m ) return x;
	double r = fmod( x, m );
	if( r < 0.0 ) r += m;
	return r < m ? r : 0.0;                                            // ( a tiny negative remainder plus m can round to m )
	}
// the map of the lane's run: freq == nullptr: the scalar for every frame
template<bool VEC>
__device__ __forceinline__ PhaseMap osc_run_map( const float * __restrict__ freq, float freq_c, int64_t f0, int len, double m )
	{
	if( len <= 0 ) return PhaseMap{ 0.0, 0.0 };
	double c = 0.0;
	if( !freq ) c = double( freq_c ) * len;
	else
		for( int i = 0; i < len; i += 4 )
			{
			float v[4];
			load4<VEC>( freq, f0 + i, len - i, v );
			#pragma unroll
			for( int k = 0; k < 4; ++k ) if( i + k < len ) c += double( v[k] );
			}
	return PhaseMap{ wrap( c, m ), m };
	}

template<bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_osc_sum( const float * __restrict__ freq, float freq_c, int64_t n, double m, int run, PhaseMap * __restrict__ tot )
	{
	__shared__ PhaseMap s_tot[SCAN_WAVES];
	int64_t f0; int len;
	lane_run( n, run, f0, len );
	PhaseMap excl, total;
	block_scan( osc_run_map<VEC>( freq, freq_c, f0, len, m ), s_tot, excl, total );
	if( threadIdx.x == 0 ) tot[blockIdx.x] = total;
	}

// phases and wave: float[n], either may be null; kind: the waveform written to `wave`
template<bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_osc_replay( const float * __restrict__ freq, float freq_c, int64_t n, double m, int run,
	const PhaseMap * __restrict__ carry, float * __restrict__ phases, float * __restrict__ wave, int kind )
	{
	__shared__ PhaseMap s_tot[SCAN_WAVES];
	int64_t f0; int len;
	lane_run( n, run, f0, len );
	PhaseMap excl, total;
	block_scan( osc_run_map<VEC>( freq, freq_c, f0, len, m ), s_tot, excl, total );
	double p = then( carry[blockIdx.x], excl ).c;                       // ( the identity's c is 0: the phase before frame 0, :57 )
	for( int i = 0; i < len; i += 4 )
		{
		float v[4] = { freq_c, freq_c, freq_c, freq_c }, ph[4], w[4];
		if( freq ) load4<VEC>( freq, f0 + i, len - i, v );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			{
			ph[k] = float( p / m );                                      // :58, one rounding
			w[k] = wave ? waveform( kind, ph[k] ) : 0.0f;
			if( i + k < len ) p = wrap( p + double( v[k] ), m );
			}
		if( phases ) store4<VEC>( phases, f0 + i, len - i, ph );
		if( wave ) store4<VEC>( wave, f0 + i, len - i, w );
		}
	}

int launch_osc( const float * d_freq, float freq, int64_t n, double m, const OscLayout & l, float * d_phases, float * d_wave, int kind, void * d_ws, hipStream_t s )
	{
	PhaseMap * tot = ws_at<PhaseMap>( d_ws, l.tot ), * carry = ws_at<PhaseMap>( d_ws, l.carry );
	auto go = [&]( auto kernel, int64_t blocks, auto... args ) { return launch_kernel( "launch_osc", kernel, blocks, SCAN_THREADS, 0, s, args... ); };
	const bool vec = l.run % 4 == 0 && n % 4 == 0 && ( !d_freq || aligned16( d_freq ) ) && ( !d_phases || aligned16( d_phases ) ) && ( !d_wave || aligned16( d_wave ) );
	if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_osc_sum<V.value>, l.blocks, d_freq, freq, n, m, l.run, tot ); } ) ) return rc;
	if( int rc = go( k_scan_carry<PhaseMap, PhaseMap>, 1, (const PhaseMap *) tot, l.blocks, carry ) ) return rc;
	return scan_pair( vec, [&]( auto V ) { return go( k_osc_replay<V.value>, l.blocks, d_freq, freq, n, m, l.run, (const PhaseMap *) carry, d_phases, d_wave, kind ); } );
	}

// Validation and sizes of synthesize_waveform (:33-46): Frame( length * sample_rate ) output frames, times oversample input frames at the fp32
// product sample_rate * oversample widened to double
struct OscSizes { int64_t num_frames = 0, n_in = 0; double in_rate = 0; };
bool osc_sizes( float length, float sample_rate, int oversample, OscSizes * z )
	{
	if( oversample < 1 || !( length > 0 ) || !( sample_rate > 0 ) ) return false;              // :33
	const float frames = length * sample_rate;                          // :39
	if( !( frames < 2147483648.0f ) ) return false;
	z->num_frames = int64_t( frames );
	z->n_in = z->num_frames * oversample;                               // :43
	z->in_rate = double( sample_rate * float( oversample ) );           // :44
	return z->num_frames > 0 && z->n_in <= INT32_MAX && std::isfinite( z->in_rate );
	}

// ---- checks -----------------------------------------------------------------------------------------------------------------------
bool shape_ok( int64_t ch, int64_t n ) { return ch > 0 && n > 0 && ch <= VOL_MAX_CHANNELS && n <= INT32_MAX; }

bool disjoint( const void * a, size_t a_bytes, const void * b, size_t b_bytes )
	{
	const uintptr_t x = reinterpret_cast<uintptr_t>( a ), y = reinterpret_cast<uintptr_t>( b );
	return x + a_bytes <= y || y + b_bytes <= x;
	}

// a pointwise output is its input's own block or shares no byte with it
int pointwise_check( const void * in, int64_t ch, int64_t n, const void * out )
	{
	FLANHIP_REQUIRE( in && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( shape_ok( ch, n ), FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	const size_t bytes = sizeof( float ) * size_t( ch ) * size_t( n );
	FLANHIP_REQUIRE( in == out || disjoint( in, bytes, out, bytes ), FLANHIP_ERR_INVALID_ARG, "the output overlaps the input without being it" );
	return FLANHIP_OK;
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int flanhip_audio_ring_modulate_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_other, int64_t other_channels,
	int64_t other_frames, float * d_out, void * stream )
	{
	if( int rc = pointwise_check( d_audio, num_channels, num_frames, d_out ) ) return rc;
	FLANHIP_REQUIRE( d_other, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( other_channels > 0 && other_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( shape_ok( other_channels, other_frames ), FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	FLANHIP_REQUIRE( disjoint( d_other, sizeof( float ) * size_t( other_channels ) * size_t( other_frames ), d_out, sizeof( float ) * size_t( num_channels ) * size_t( num_frames ) ),
		FLANHIP_ERR_INVALID_ARG, "the output overlaps the modulator" );
	if( int rc = require_device() ) return rc;
	const RingOp op{ d_other, uint32_t( other_channels ), uint32_t( other_frames ) };
	return launch_pointwise( "flanhip_audio_ring_modulate_dev", d_audio, d_out, num_frames, num_channels * num_frames, op, (hipStream_t) stream );
	}

int flanhip_fade_frames_plan( int64_t num_frames, int32_t start, int32_t end, int32_t * out2 )
	{
	FLANHIP_REQUIRE( out2, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	start = std::max( 0, start );                                        // AudioVolume.cpp:111-112
	end = std::max( 0, end );
	if( int64_t( start ) + int64_t( end ) > num_frames )                 // :113-118 (the sum in 64 bits: the reference's int overflows there)
		{
		const float scale = float( num_frames ) / float( int64_t( start ) + int64_t( end ) );
		start = int32_t( std::floor( float( start ) * scale ) );
		end = int32_t( std::floor( float( end ) * scale ) );
		// fp32 may round a product up to the next whole frame: what the two loops then do twice over stays inside the frames
		start = int32_t( std::min<int64_t>( start, num_frames ) );
		end = int32_t( std::min<int64_t>( end, num_frames ) );
		}
	out2[0] = start; out2[1] = end;
	return FLANHIP_OK;
	}

int flanhip_audio_fade_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_start_gain, int64_t start,
	const float * d_end_gain, int64_t end, float * d_out, void * stream )
	{
	if( int rc = pointwise_check( d_audio, num_channels, num_frames, d_out ) ) return rc;
	FLANHIP_REQUIRE( start >= 0 && end >= 0 && start <= num_frames && end <= num_frames, FLANHIP_ERR_INVALID_ARG, "a fade outside the frames" );
	FLANHIP_REQUIRE( ( d_start_gain || start == 0 ) && ( d_end_gain || end == 0 ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	const size_t bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames );
	FLANHIP_REQUIRE( ( start == 0 || disjoint( d_start_gain, sizeof( float ) * size_t( start ), d_out, bytes ) )
		&& ( end == 0 || disjoint( d_end_gain, sizeof( float ) * size_t( end ), d_out, bytes ) ), FLANHIP_ERR_INVALID_ARG, "the output overlaps a gain table" );
	if( int rc = require_device() ) return rc;
	const FadeOp op{ d_start_gain, d_end_gain, num_frames, start, end };
	return launch_pointwise( "flanhip_audio_fade_dev", d_audio, d_out, num_frames, num_channels * num_frames, op, (hipStream_t) stream );
	}

int flanhip_audio_moisture_dev( const float * d_oversampled, int64_t num_channels, int64_t oversampled_frames, float oversampled_rate, int64_t num_frames,
	float sample_rate, const float * d_amount, float amount, const float * d_frequency, float frequency, const float * d_skew, float skew, int waveform_kind,
	float * d_out, void * stream )
	{
	if( int rc = pointwise_check( d_oversampled, num_channels, oversampled_frames, d_out ) ) return rc;
	FLANHIP_REQUIRE( num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( oversampled_rate > 0.0f && sample_rate > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( valid_waveform( waveform_kind ), FLANHIP_ERR_INVALID_ARG, "not a named waveform" );
	if( int rc = require_device() ) return rc;
	const MoistOp op{ d_amount, d_frequency, d_skew, amount, frequency, skew, oversampled_rate, sample_rate, num_frames, waveform_kind };
	return launch_pointwise( "flanhip_audio_moisture_dev", d_oversampled, d_out, oversampled_frames, num_channels * oversampled_frames, op, (hipStream_t) stream );
	}

int flanhip_waveform_dev( int waveform_kind, const float * d_t, int64_t count, float * d_out, void * stream )
	{
	FLANHIP_REQUIRE( d_t && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( count <= ( int64_t( 1 ) << 40 ), FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	FLANHIP_REQUIRE( valid_waveform( waveform_kind ), FLANHIP_ERR_INVALID_ARG, "not a named waveform" );
	FLANHIP_REQUIRE( d_t == d_out || disjoint( d_t, sizeof( float ) * size_t( count ), d_out, sizeof( float ) * size_t( count ) ), FLANHIP_ERR_INVALID_ARG,
		"the output overlaps the input without being it" );
	if( int rc = require_device() ) return rc;
	return launch_pointwise( "flanhip_waveform_dev", d_t, d_out, count, count, WaveOp{ waveform_kind }, (hipStream_t) stream );
	}

int flanhip_waveform_host( int waveform_kind, const float * t, int64_t count, float * out )
	{
	FLANHIP_REQUIRE( t && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( valid_waveform( waveform_kind ), FLANHIP_ERR_INVALID_ARG, "not a named waveform" );
	for( int64_t i = 0; i < count; ++i ) out[i] = waveform_host( waveform_kind, t[i] );
	return FLANHIP_OK;
	}

size_t flanhip_audio_energy_workspace_bytes( int64_t num_channels, int64_t num_frames )
	{
	if( !shape_ok( num_channels, num_frames ) ) return 0;
	return ( sizeof( double ) * size_t( num_channels ) * size_t( energy_blocks( num_frames ) ) + 255 ) & ~size_t( 255 );
	}

int flanhip_audio_energy_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_energy, void * d_workspace, void * stream )
	{
	FLANHIP_REQUIRE( d_audio && d_energy, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_channels > 0 && num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( shape_ok( num_channels, num_frames ), FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	const int64_t blocks = energy_blocks( num_frames );
	double * partial = static_cast<double*>( d_workspace );
	if( int rc = launch_kernel( "flanhip_audio_energy_dev", k_energy, num_channels * blocks, VOL_THREADS, 0, (hipStream_t) stream, d_audio, num_frames, blocks, partial ) ) return rc;
	return launch_kernel( "flanhip_audio_energy_dev", k_energy_close, num_channels, VOL_THREADS, 0, (hipStream_t) stream, (const double *) partial, blocks, d_energy );
	}

int flanhip_audio_rectify_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_out, void * stream )
	{
	if( int rc = pointwise_check( d_audio, num_channels, num_frames, d_out ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_pointwise( "flanhip_audio_rectify_dev", d_audio, d_out, num_frames, num_channels * num_frames, RectOp{}, (hipStream_t) stream );
	}

// ---- the oscillator -----------------------------------------------------------------------------------------------------------------
void flanhip_osc_debug_run( int frames ) { t_osc_run = frames > 0 ? frames : 0; }
int64_t flanhip_osc_run_frames( void ) { return scan_run( t_osc_run ); }
int64_t flanhip_osc_block_frames( void ) { return int64_t( scan_run( t_osc_run ) ) * SCAN_THREADS; }
int64_t flanhip_osc_carry_pass_blocks( void ) { return SCAN_THREADS; }

size_t flanhip_osc_workspace_bytes( int64_t num_in_frames )
	{
	OscLayout l;
	if( !osc_layout( num_in_frames, &l ) ) return 0;
	return l.total;
	}

int flanhip_osc_phase_dev( const float * d_freq, float freq, int64_t num_in_frames, double in_sample_rate, float * d_phases, float * d_wave, int waveform_kind,
	void * d_workspace, void * stream )
	{
	FLANHIP_REQUIRE( num_in_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_in_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( in_sample_rate > 0.0 && std::isfinite( in_sample_rate ), FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( d_phases || d_wave, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( !d_wave || valid_waveform( waveform_kind ), FLANHIP_ERR_INVALID_ARG, "not a named waveform" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	OscLayout l;
	FLANHIP_REQUIRE( osc_layout( num_in_frames, &l ), FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	if( int rc = require_device() ) return rc;
	return launch_osc( d_freq, freq, num_in_frames, in_sample_rate, l, d_phases, d_wave, waveform_kind, d_workspace, (hipStream_t) stream );
	}

int64_t flanhip_synthesize_waveform_frames( float length, float sample_rate, int oversample, int64_t * num_in_frames, double * in_sample_rate )
	{
	OscSizes z;
	if( !osc_sizes( length, sample_rate, oversample, &z ) ) return -1;
	if( num_in_frames ) *num_in_frames = z.n_in;
	if( in_sample_rate ) *in_sample_rate = z.in_rate;
	return z.num_frames;
	}

int flanhip_oneshot_resample_dev( const float * d_in, int64_t num_in_frames, double src_rate, double dst_rate, float * d_out, int64_t num_out_frames, void * stream )
	{
	FLANHIP_REQUIRE( d_in && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_in_frames > 0 && num_out_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_in_frames <= INT32_MAX && num_out_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( src_rate > 0.0 && dst_rate > 0.0, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	const bool equal = src_rate == dst_rate;
	FLANHIP_REQUIRE( equal || resample_chain_served( src_rate, dst_rate ), FLANHIP_ERR_UNSUPPORTED, "no chain of r8brain's stages for these rates" );
	if( int rc = require_device() ) return rc;
	hipStream_t s = (hipStream_t) stream;
	if( !equal ) return resample_chain_dev( d_in, num_in_frames, src_rate, dst_rate, d_out, num_out_frames, s );
	// CDSPResampler.h:133-136: no steps: process() hands the input back, and oneshot feeds zeros once the input is used up
	const int64_t copied = std::min( num_in_frames, num_out_frames );
	FLANHIP_CHECK( hipMemcpyAsync( d_out, d_in, sizeof( float ) * size_t( copied ), hipMemcpyDeviceToDevice, s ) );
	if( copied < num_out_frames ) FLANHIP_CHECK( hipMemsetAsync( d_out + copied, 0, sizeof( float ) * size_t( num_out_frames - copied ), s ) );
	return FLANHIP_OK;
	}

// the workspace: the scan's tables, then the wave samples float[n_in]
size_t flanhip_audio_synthesize_waveform_workspace_bytes( float length, float sample_rate, int oversample )
	{
	OscSizes z; OscLayout l;
	if( !osc_sizes( length, sample_rate, oversample, &z ) || !osc_layout( z.n_in, &l ) ) return 0;
	return l.total + ( ( sizeof( float ) * size_t( z.n_in ) + 255 ) & ~size_t( 255 ) );
	}

int flanhip_audio_synthesize_waveform_dev( int waveform_kind, const float * d_freq, float freq, float length, float sample_rate, int oversample, float * d_out,
	void * d_workspace, void * stream )
	{
	OscSizes z; OscLayout l;
	FLANHIP_REQUIRE( osc_sizes( length, sample_rate, oversample, &z ) && osc_layout( z.n_in, &l ), FLANHIP_ERR_INVALID_ARG, "oversample < 1, length <= 0, sample_rate <= 0 or too many frames" );
	FLANHIP_REQUIRE( valid_waveform( waveform_kind ), FLANHIP_ERR_INVALID_ARG, "not a named waveform" );
	FLANHIP_REQUIRE( d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	FLANHIP_REQUIRE( z.in_rate == double( sample_rate ) || resample_chain_served( z.in_rate, double( sample_rate ) ), FLANHIP_ERR_UNSUPPORTED, "no chain of r8brain's stages for these rates" );
	if( int rc = require_device() ) return rc;
	float * d_wave = ws_at<float>( d_workspace, l.total );
	if( int rc = launch_osc( d_freq, freq, z.n_in, z.in_rate, l, nullptr, d_wave, waveform_kind, d_workspace, (hipStream_t) stream ) ) return rc;
	return flanhip_oneshot_resample_dev( d_wave, z.n_in, z.in_rate, double( sample_rate ), d_out, z.num_frames, stream );      // :65-66
	}

int flanhip_white_noise_draw( uint64_t seed, int64_t count, float * out )
	{
	FLANHIP_REQUIRE( out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	std::mt19937 rng( static_cast<uint32_t>( seed ) );                  // AudioSynthesis.cpp:81-86
	std::uniform_real_distribution<> dis( -1.0f, 1.0f );
	for( int64_t i = 0; i < count; ++i ) out[i] = float( dis( rng ) );
	return FLANHIP_OK;
	}

} // extern "C"
