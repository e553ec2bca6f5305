// AudioBuffer.cpp -- host/device mirrored audio container (reference: src/flan/Audio/AudioBuffer.cpp:17-29,479-482).
#include "flan/AudioBuffer.h"

#include <algorithm>
#include <utility>

#include <cmath>
#include <iostream>

namespace flan {

AudioBuffer::AudioBuffer() : format() {}

AudioBuffer::AudioBuffer( const Format & other ) : format( other ), mirror( "audio", false, std::vector<float>( count() ) ) {}

AudioBuffer::AudioBuffer( std::vector<float> && temp_buffer, Channel num_channels, FrameRate sr )
	: format{ num_channels, num_channels > 0 ? Frame( temp_buffer.size() / num_channels ) : 0, sr }   // AudioBuffer.cpp:22
	, mirror( "audio", false, std::move( temp_buffer ) )
	{}

AudioBuffer AudioBuffer::adopt_device( const Format & f, std::shared_ptr<detail::DeviceBlock> block )
	{
	AudioBuffer out;
	out.format = f;
	out.mirror.adopt( std::move( block ) );
	return out;
	}

AudioBuffer AudioBuffer::copy() const
	{
	AudioBuffer out;
	out.format = format;
	out.mirror = mirror.copy( count() );   // deep copy of the samples
	return out;
	}

bool AudioBuffer::is_null() const { return count() == 0 || mirror.holds_nothing() || format.sample_rate == 0; }

void AudioBuffer::clear_buffer() { mirror.clear( count() ); }

Sample AudioBuffer::get_sample( Channel c, Frame f ) const { return get_buffer()[get_buffer_pos( c, f )]; }
Sample & AudioBuffer::get_sample( Channel c, Frame f ) { return get_buffer()[get_buffer_pos( c, f )]; }
void AudioBuffer::set_sample( Channel c, Frame f, Sample s ) { get_buffer()[get_buffer_pos( c, f )] = s; }

bool AudioBuffer::is_nan_or_inf() const
	{
	for( float v : get_buffer() ) if( std::isnan( v ) || std::isinf( v ) ) return true;   // AudioBuffer.cpp:58-64
	return false;
	}

Sample AudioBuffer::get_max_sample_magnitude( Second start_time, Second end_time ) const
	{
	if( get_num_frames() <= 0 ) return 0;
	if( end_time == 0 ) end_time = get_length();                                  // AudioBuffer.cpp:418-420
	const Frame start_frame = std::clamp( Frame( time_to_frame( start_time ) ), 0, get_num_frames() - 1 );
	const Frame end_frame = std::clamp( Frame( time_to_frame( end_time ) ), 0, get_num_frames() - 1 );
	const std::vector<float> & data = get_buffer();
	Magnitude m = 0;
	for( Channel channel = 0; channel < get_num_channels(); ++channel )
		for( Frame frame = start_frame; frame < end_frame; ++frame )
			m = std::max( m, std::abs( data[get_buffer_pos( channel, frame )] ) );
	return m;
	}

void AudioBuffer::print_summary() const
	{
	std::cout << "\n=========================== Audio Info ==========================="       // AudioBuffer.cpp:500-509
	          << "\nChannels:\t" << get_num_channels() << "\nSamples:\t" << get_num_frames() << "\nSample Rate:\t" << get_sample_rate()
	          << "\n==================================================================" << "\n\n";
	}

} // namespace flan
